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
//   articulated bodies (eg_articulate_check, eg_articulate_levels, eg_articulate_forward, eg_articulate_rot6d): tracks of 6-D joint rotations
//             (pose_dim = 6J) -> joint positions and joint rotations in one launch, on the same tile walk with a tile height of its own, and the
//             elementwise inverse; see the section further down.
//   Euler channels (eg_articulate_euler, eg_articulate_rot6d_euler): the same tracks -> the angles of every joint's BVH rotation channels, on the
//             articulate kernel's tile walk without the level walk, and the elementwise inverse; see the section further down.  The Euler
//             filter over the angles is csrc/euler.hip.
#include "rows.h"
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
__device__ __forceinline__ void stage_quads(const float* __restrict__ base, long long g0, long long g1, long long total, float* lds) {
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

template <bool NATIVE, int TILE = TF>
__device__ __forceinline__ Tile tile_of(const Args& a, long long T_out) {
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const long long k0 = (long long)tile * TILE;
    const int cnt = (int)(T_out - k0 < TILE ? T_out - k0 : TILE);
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const long long n_out = NATIVE ? n : out_frames(n, a.L, a.M);
    const long long live = n_out - k0 < 0 ? 0 : (n_out - k0 < cnt ? n_out - k0 : cnt);
    return {b, k0, cnt, n, live, (int)live};
}

// Zeros in the frames [live, cnt) of a tile whose frames have `row` floats and start at float out0.
__device__ __forceinline__ void zero_tail(float* __restrict__ dst, long long out0, int row, const Tile& t) {
    if (t.live < t.cnt) store_range(dst, out0, row, out0 + t.live64 * row, out0 + (long long)t.cnt * row, [](int, int) { return 0.f; });
}

// The window form of the forward kernels (eg_*_window: a stream's delayed output stage, csrc/render_stream.hip).  A row is a window of source
// frames, and two things are new.  The output limit: a.T_out may be less than ceil(T L / M), and `cnt` above already cuts `live` there.  The
// zeroed head: a.frames holds two ints per row, [2][B] -- the window's valid frames, which egi_valid_frames reads as ever (draws = 1), then
// the number of leading output frames that are written as zeros.  Returns that number inside the tile, 0..live; the frames below it are
// computed like the others (from finite source frames) and replaced by zeros where they are stored.  WINDOW = false: nothing, no code.
template <bool WINDOW>
__device__ __forceinline__ int zero_head(const Args& a, const Tile& t) {
    if (!WINDOW) return 0;
    const long long h = (long long)a.frames[a.B + t.b] - t.k0;
    return (int)(h < 0 ? 0 : (h < t.live ? h : t.live));
}

// The source frames of a tile of the forward kernels.  A pass makes the outputs [i, i1) of the tile from the source frames
// [s_base, s_base + nslots): as many outputs as SL source frames reach (all of them unless the rate drops, M > L).  SL: the tile height + 2.
struct Pass { long long s_base; int i1, nslots; };
struct Blend { int slot; float f; };                    // output = frame(slot) + (frame(slot + 1) - frame(slot)) * f, slots counted from s_base

template <bool NATIVE, int SL = SLOTS>
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
            const long long jmax = ((s_base + SL - 1) * L - 1) / M - k0;        // last output whose segment starts at or before s_base + SL - 2
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
template <bool NATIVE, int SL = SLOTS>
__device__ __forceinline__ float* stage_pass(const Args& a, const Tile& t, const Walk<NATIVE, SL>& w, int i, float* xin, Pass& p) {
    const int D = 3 * a.K;
    p = w.pass(i, t.live);
    const long long g0 = ((long long)t.b * a.T + p.s_base) * D;
    stage_quads(a.src, g0, g0 + (long long)p.nslots * D, (long long)a.B * a.T * D, xin);
    __syncthreads();
    return xin + (int)(g0 & 3);
}

// NATIVE: L / M = 1.  WINDOW: the window form (zero_head).
template <bool UNIT, bool NATIVE, bool WINDOW = false>
__global__ __launch_bounds__(THREADS) void skeleton_joints_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = a.K, D = 3 * K, J3 = 3 * (K + 1), tid = threadIdx.x;
    float* xin = lds + HEAD;
    float* pj = xin + round4(SLOTS * D + 8);
    const Tile t = tile_of<NATIVE>(a, a.T_out);
    const long long out0 = ((long long)t.b * a.T_out + t.k0) * J3;
    zero_tail(a.dst, out0, J3, t);
    if (t.live == 0) return;
    const int zh = zero_head<WINDOW>(a, t);
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
            if (WINDOW && fr < zh) return 0.f;
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
    stage_quads(a.src, g0, g0 + (long long)t.live * J3, (long long)a.B * a.T * J3, pin);
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
template <bool NATIVE, bool GLOBAL, bool WINDOW = false>
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
    const int zh = zero_head<WINDOW>(a, t);
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
                if (WINDOW && fr < zh) *reinterpret_cast<f4*>(out + ((long long)fr * K + k) * 4) = f4{0.f, 0.f, 0.f, 0.f};
                else *reinterpret_cast<f4*>(out + ((long long)fr * K + k) * 4) = f4{o.w, o.x, o.y, o.z};
            }
            __syncthreads();                                                    // a level reads what the level before wrote
        }
    }
}

// ---- articulated bodies: 6-D joint rotations -> joints and rotations (eg_articulate_*) ---------------------------------------------------------
// The rotations kernel's grid, staging and level walk on a tile of TFA output frames; the state of a joint is its global rotation as a matrix
// and its position, 12 floats in an LDS tile st[joint][component][frame] (the chain is then the definition's own sequence of products, and a
// degenerate group stays what the definition says).  A pass has two phases: R_j of every (frame, joint) at once -- Gram-Schmidt with its
// square roots and divisions has no parent -- then the level walk, which only multiplies (skipped when nothing asks for G or p).  A joint's plane has AST = 13 rows of TFA floats: the spare row keeps the joints of a level
// off each other's banks.  The six numbers of a joint are read straight from the staged quads -- no second copy -- so the staged frames
// ((TFA + 2) x 6J floats) and the state (J x AST) share the workgroup's LDS about evenly: 45 KiB at J = 64, 34 KiB at J = 47.
// The level table of eg_articulate_levels: the level count | ALEVELS level offsets | order [J] | parents [J] | offsets [3J].
constexpr int TFA = EG_ARTICULATE_TILE_FRAMES;
constexpr int SLA = TFA + 2;
constexpr int MAX_J = EG_ARTICULATE_MAX_JOINTS;
constexpr int ALEVELS = MAX_J + 1;                      // a level per joint at most, and the offset behind the last one
constexpr int AL_FIRST = 1, AL_ORDER = AL_FIRST + ALEVELS;
__host__ __device__ constexpr int al_parents(int J) { return AL_ORDER + J; }
__host__ __device__ constexpr int al_offsets(int J) { return AL_ORDER + 2 * J; }
static_assert(al_offsets(1) + 3 == EG_ARTICULATE_LEVEL_WORDS(1) && al_offsets(MAX_J) + 3 * MAX_J == EG_ARTICULATE_LEVEL_WORDS(MAX_J), "the header's table size");
constexpr int AL_OFFS = round4(ALEVELS);                // LDS words: level offsets [nlev + 1 <= ALEVELS] (+ pad)
constexpr int AHEAD = AL_OFFS + 2 * MAX_J + 3 * MAX_J + 6 * MAX_J;      // offsets | order | parents | offsets [3 * 64] | mean [6 * 64]
constexpr int AST = 13 * TFA;
static_assert(AHEAD % 4 == 0, "the staged frames start on a quad");
static_assert((AHEAD + round4(SLA * 6 * MAX_J + 8) + MAX_J * AST) * sizeof(float) <= 64 * 1024, "a workgroup's LDS at J = 64");
constexpr int TFI = 16;                                 // frames of one workgroup of the inverse

// Args::K counts the 3-vectors of a source frame, 2J: stage_pass and load_mean then see rows of 3K = 6J floats.
struct ArtArgs { Args a; float* rot; int J, columns; };

// quat(m) of the header: the branch of the first largest of (trace, m00, m11, m22), normalised, w >= 0.
__device__ __forceinline__ f4 quat_of(const float* m) {
    const float tr = m[0] + m[4] + m[8];
    float w, x, y, z;
    if (tr >= m[0] && tr >= m[4] && tr >= m[8]) { w = 1.f + tr; x = m[7] - m[5]; y = m[2] - m[6]; z = m[3] - m[1]; }
    else if (m[0] >= m[4] && m[0] >= m[8]) { w = m[7] - m[5]; x = 1.f + m[0] - m[4] - m[8]; y = m[1] + m[3]; z = m[2] + m[6]; }
    else if (m[4] >= m[8]) { w = m[2] - m[6]; x = m[1] + m[3]; y = 1.f - m[0] + m[4] - m[8]; z = m[5] + m[7]; }
    else { w = m[3] - m[1]; x = m[2] + m[6]; y = m[5] + m[7]; z = 1.f - m[0] - m[4] + m[8]; }
    float d = fmaxf(sqrtf(w * w + x * x + y * y + z * z), 1e-12f);
    if (w < 0.f) d = -d;
    return f4{w / d, x / d, y / d, z / d};
}

// R_j of output frame fr of the tile (frame fl of the pass ps, staged at x in rows of D floats): the six numbers of joint j (+ mean), blended
// where the rate changes, then Gram-Schmidt.  The one definition behind the joints, the quaternions and the Euler angles of a pose.
template <bool NATIVE, int SL>
__device__ __forceinline__ void rot6d_matrix(const float* x, const Walk<NATIVE, SL>& w, const Pass& ps, int fl, int fr, int j, int D, const float* mn,
                                             bool has_mean, int columns, float (&R)[9]) {
    const float* mj = mn + 6 * j;                                              // once: written as mn[6 * j + e] the address is remade per element
    float d[6];
    if (NATIVE || w.n < 2) {
        const float* xs = x + (NATIVE ? fl : 0) * D + 6 * j;
#pragma unroll
        for (int e = 0; e < 6; ++e) d[e] = has_mean ? xs[e] + mj[e] : xs[e];
    } else {                                                                    // the 6-D vectors are blended, after the mean
        const Blend bl = w.blend(ps, fr);
        const float* xs = x + bl.slot * D + 6 * j;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            float y = xs[e], z = xs[D + e];
            if (has_mean) { y += mj[e]; z += mj[e]; }
            d[e] = fmaf(z - y, bl.f, y);
        }
    }
    const float n1 = fmaxf(sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), 1e-12f);
    const float b10 = d[0] / n1, b11 = d[1] / n1, b12 = d[2] / n1;
    const float dot = b10 * d[3] + b11 * d[4] + b12 * d[5];
    const float u0 = d[3] - dot * b10, u1 = d[4] - dot * b11, u2 = d[5] - dot * b12;
    const float n2 = fmaxf(sqrtf(u0 * u0 + u1 * u1 + u2 * u2), 1e-12f);
    const float b20 = u0 / n2, b21 = u1 / n2, b22 = u2 / n2;
    const float b30 = b11 * b22 - b12 * b21, b31 = b12 * b20 - b10 * b22, b32 = b10 * b21 - b11 * b20;
    if (columns) { R[0] = b10; R[1] = b20; R[2] = b30; R[3] = b11; R[4] = b21; R[5] = b31; R[6] = b12; R[7] = b22; R[8] = b32; }
    else { R[0] = b10; R[1] = b11; R[2] = b12; R[3] = b20; R[4] = b21; R[5] = b22; R[6] = b30; R[7] = b31; R[8] = b32; }
}

// NATIVE: L / M = 1.  GLOBAL: the rotations hold G_j, else R_j.  a.dst: the joints or null; k.rot: the rotations or null.
template <bool NATIVE, bool GLOBAL, bool WINDOW = false>
__global__ __launch_bounds__(THREADS) void articulate_kernel(const ArtArgs k) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Args& a = k.a;
    const int J = k.J, D = 6 * J, J3 = 3 * J, tid = threadIdx.x;
    int* lv = reinterpret_cast<int*>(lds);
    int* ord = lv + AL_OFFS;
    int* par = ord + MAX_J;
    float* off = lds + AL_OFFS + 2 * MAX_J;
    float* mn = off + 3 * MAX_J;
    float* xin = lds + AHEAD;
    float* st = xin + round4(SLA * D + 8);                                      // st[joint][component][frame of the tile]
    const Tile t = tile_of<NATIVE, TFA>(a, a.T_out);
    const long long f0 = (long long)t.b * a.T_out + t.k0;                       // the tile's first output frame
    if (a.dst) zero_tail(a.dst, f0 * J3, J3, t);
    float* rot = k.rot ? k.rot + f0 * 4 * J : nullptr;                          // 16-byte aligned: every joint is a quad
    if (rot)
        for (int q = t.live * J + tid; q < t.cnt * J; q += THREADS) *reinterpret_cast<f4*>(rot + 4ll * q) = f4{0.f, 0.f, 0.f, 0.f};
    if (t.live == 0) return;
    const int zh = zero_head<WINDOW>(a, t);
    const int nlev = min(max(a.table[0], 1), J);
    for (int l = tid; l <= nlev; l += THREADS) lv[l] = min(max(a.table[AL_FIRST + l], 0), J);
    for (int j = tid; j < J; j += THREADS) {
        ord[j] = min(max(a.table[AL_ORDER + j], 0), J - 1);
        par[j] = min(max(a.table[al_parents(J) + j], -1), J - 1);
    }
    for (int r = tid; r < J3; r += THREADS) off[r] = __int_as_float(a.table[al_offsets(J) + r]);
    const bool has_mean = a.mean != nullptr;
    load_mean(a, mn);
    // stage_pass' barrier also covers the tables, and the last level of the pass before
    const Walk<NATIVE, SLA> w = {t.k0, t.n, a.L, a.M};
    Pass ps;
    for (int i = 0; i < t.live; i = ps.i1) {
        const float* x = stage_pass(a, t, w, i, xin, ps);
        const int nf = ps.i1 - i;
        // Phase 1, every (output frame, joint) at once: R_j by Gram-Schmidt into the joint's own plane of the state tile; the local rotations leave here.
        for (int q = tid; q < nf * J; q += THREADS) {
            const int j = q / nf, fr = i + (q - j * nf);
            float R[9];
            rot6d_matrix(x, w, ps, fr - i, fr, j, D, mn, has_mean, k.columns, R);
            float* sj = st + j * AST + fr;
#pragma unroll
            for (int e = 0; e < 9; ++e) sj[e * TFA] = R[e];
            if (!GLOBAL && rot) {
                if (WINDOW && fr < zh) *reinterpret_cast<f4*>(rot + ((long long)fr * J + j) * 4) = f4{0.f, 0.f, 0.f, 0.f};
                else *reinterpret_cast<f4*>(rot + ((long long)fr * J + j) * 4) = quat_of(R);
            }
        }
        __syncthreads();                                                        // xin is free from here on; the chain reads R from the tile
        // Phase 2, the chain, only where something needs it: G_j replaces R_j in the joint's plane (its owner reads R_j and writes G_j; nobody
        // else touches the plane before the barrier), the position goes beside it.  The dependent path is 36 multiply-adds per level.
        const int walk = (a.dst || (GLOBAL && rot)) ? nlev : 0;
        for (int l = 0; l < walk; ++l) {
            const int b0 = lv[l], nb = max(lv[l + 1] - b0, 0);
            for (int q = tid; q < nf * nb; q += THREADS) {                       // one thread per (output frame, joint of the level)
                const int jl = q / nf, fr = i + (q - jl * nf);
                const int j = ord[min(b0 + jl, J - 1)], p = par[j];
                float* sj = st + j * AST + fr;
                float R[9], G[9], pos[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) R[e] = sj[e * TFA];
                const float o0 = off[3 * j], o1 = off[3 * j + 1], o2 = off[3 * j + 2];
                if (p >= 0) {
                    const float* sp = st + p * AST + fr;
                    float P[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) P[e] = sp[e * TFA];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) G[3 * r + c] = P[3 * r] * R[c] + P[3 * r + 1] * R[3 + c] + P[3 * r + 2] * R[6 + c];
                        pos[r] = sp[(9 + r) * TFA] + (P[3 * r] * o0 + P[3 * r + 1] * o1 + P[3 * r + 2] * o2);
                    }
#pragma unroll
                    for (int e = 0; e < 9; ++e) sj[e * TFA] = G[e];
                } else {                                                        // the root: G = R is in place already
#pragma unroll
                    for (int e = 0; e < 9; ++e) G[e] = R[e];
                    pos[0] = o0; pos[1] = o1; pos[2] = o2;
                }
#pragma unroll
                for (int e = 0; e < 3; ++e) sj[(9 + e) * TFA] = pos[e];
                if (GLOBAL && rot) {
                    if (WINDOW && fr < zh) *reinterpret_cast<f4*>(rot + ((long long)fr * J + j) * 4) = f4{0.f, 0.f, 0.f, 0.f};
                    else *reinterpret_cast<f4*>(rot + ((long long)fr * J + j) * 4) = quat_of(G);
                }
            }
            __syncthreads();                                                    // a level reads what the level before wrote
        }
        if (a.dst)                                                              // the positions of the pass, from the state tile
            store_range(a.dst, f0 * J3, J3, (f0 + i) * J3, (f0 + ps.i1) * J3, [&](int fr, int r) {
                const int jt = r / 3;
                if (WINDOW && fr < zh) return 0.f;
                return st[jt * AST + (9 + r - 3 * jt) * TFA + fr];
            });
    }
}

// The frame of both inverse kernels, anything [B, T, J, .] -> rot6d [B, T, 6J] on tiles of TFI frames: the zero tail, the mean, then
// fill(n, q0) leaves the six floats of the tile's n (frame, joint) pairs in buf[6 q] -- pair q is pair q0 + q of the whole input, the tile's
// rows are contiguous -- and they leave through store_range minus the mean, coalesced.
template <class F>
__device__ __forceinline__ void rot6d_tile(const Args& a, int J, float* mn, const float* buf, F fill) {
    const int D = 6 * J;
    const Tile t = tile_of<true, TFI>(a, a.T);
    const long long f0 = (long long)t.b * a.T + t.k0;
    zero_tail(a.dst, f0 * D, D, t);
    if (t.live == 0) return;
    const bool has_mean = a.mean != nullptr;
    load_mean(a, mn);
    fill(t.live * J, f0 * J);
    __syncthreads();
    store_range(a.dst, f0 * D, D, f0 * D, (f0 + t.live) * D, [&](int fr, int r) {
        const float v = buf[fr * D + r];
        return has_mean ? v - mn[r] : v;
    });
}

// quat [B, T, J, 4] -> rot6d [B, T, 6J]: one 16-byte load per (frame, joint).
__global__ __launch_bounds__(THREADS) void articulate_rot6d_kernel(const ArtArgs k) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Args& a = k.a;
    float* buf = lds + 6 * MAX_J;
    rot6d_tile(a, k.J, lds, buf, [&](int n, long long q0) {
        for (int q = threadIdx.x; q < n; q += THREADS) {
            const f4 v = *reinterpret_cast<const f4*>(a.src + (q0 + q) * 4);
            const float d = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]), 1e-12f);
            const float w = v[0] / d, x = v[1] / d, y = v[2] / d, z = v[3] / d;
            const float m00 = 1.f - 2.f * (y * y + z * z), m01 = 2.f * (x * y - w * z), m02 = 2.f * (x * z + w * y);
            const float m10 = 2.f * (x * y + w * z), m11 = 1.f - 2.f * (x * x + z * z), m12 = 2.f * (y * z - w * x);
            float* o = buf + 6 * q;
            if (k.columns) { o[0] = m00; o[1] = m10; o[2] = 2.f * (x * z - w * y); o[3] = m01; o[4] = m11; o[5] = 2.f * (y * z + w * x); }
            else { o[0] = m00; o[1] = m01; o[2] = m02; o[3] = m10; o[4] = m11; o[5] = m12; }
        }
    });
}

// ---- Euler channels (eg_articulate_euler, eg_articulate_rot6d_euler) ------------------------------------------------------------------------
// No tree walk: R_j of every (output frame, joint) by the articulate kernel's own Gram-Schmidt, three angles from it, 12 bytes into an LDS tile
// eo[frame][joint][3] that leaves through store_range as whole rows.  An order code is 2 i + (descending): XYZ XZY YXZ YZX ZXY ZYX = 0..5;
// the seven (inverse: six) entries a thread needs are picked from its nine registers by selects, so joints of different orders in one wave
// run the same instructions.  The device table of codes indexes nothing but the selects; it is clamped to 0..5 all the same.
constexpr int EHEAD = MAX_J + 6 * MAX_J;                // order codes | mean [6 * 64]
static_assert(EHEAD % 4 == 0, "the staged frames start on a quad");

struct EulArgs { Args a; const int* orders; int J, columns; float scale; };     // scale: forward rad -> output unit; inverse: input unit -> rad

__device__ __forceinline__ float pick9(const float* m, int idx) {
    float v = m[0];
#pragma unroll
    for (int e = 1; e < 9; ++e) v = idx == e ? m[e] : v;
    return v;
}

struct Axes { int i, j, k; float eps; };
__device__ __forceinline__ Axes order_axes(int code) {
    const int i = code >> 1, lo = i == 0 ? 1 : 0, hi = i == 2 ? 1 : 2;
    const int j = (code & 1) ? hi : lo, k = (code & 1) ? lo : hi;
    return {i, j, k, j == (i == 2 ? 0 : i + 1) ? 1.f : -1.f};
}

template <bool NATIVE, bool WINDOW = false>
__global__ __launch_bounds__(THREADS) void articulate_euler_kernel(const EulArgs k) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Args& a = k.a;
    const int J = k.J, D = 6 * J, J3 = 3 * J, tid = threadIdx.x;
    int* ord = reinterpret_cast<int*>(lds);
    float* mn = lds + MAX_J;
    float* xin = lds + EHEAD;
    float* eo = xin + round4(SLA * D + 8);                                      // eo[frame of the tile][joint][3]
    const Tile t = tile_of<NATIVE, TFA>(a, a.T_out);
    const long long f0 = (long long)t.b * a.T_out + t.k0;
    zero_tail(a.dst, f0 * J3, J3, t);
    if (t.live == 0) return;
    const int zh = zero_head<WINDOW>(a, t);
    for (int j = tid; j < J; j += THREADS) ord[j] = min(max(k.orders[j], 0), 5);
    const bool has_mean = a.mean != nullptr;
    load_mean(a, mn);
    // stage_pass' barrier also covers the tables; the barrier behind the angles ended the reads of xin, and a later pass writes other frames of eo
    const Walk<NATIVE, SLA> w = {t.k0, t.n, a.L, a.M};
    Pass ps;
    for (int i = 0; i < t.live; i = ps.i1) {
        const float* x = stage_pass(a, t, w, i, xin, ps);
        const int nf = ps.i1 - i;
        for (int q = tid; q < nf * J; q += THREADS) {                            // one thread per (output frame, joint)
            const int fl = q / J, j = q - fl * J, fr = i + fl;
            float R[9];
            rot6d_matrix(x, w, ps, fl, fr, j, D, mn, has_mean, k.columns, R);
            const Axes o = order_axes(ord[j]);
            const float rii = pick9(R, 4 * o.i), rij = pick9(R, 3 * o.i + o.j), s = o.eps * pick9(R, 3 * o.i + o.k);
            const float eb = atan2f(s, sqrtf(rii * rii + rij * rij));
            float ea, ec;
            if (1.f - fabsf(s) >= 0x1p-20f) {
                ea = atan2f(-o.eps * pick9(R, 3 * o.j + o.k), pick9(R, 4 * o.k));
                ec = atan2f(-o.eps * rij, rii);
            } else {                                                            // the lock: a and c turn about one axis, c = 0
                ea = atan2f(o.eps * pick9(R, 3 * o.k + o.j), pick9(R, 4 * o.j));
                ec = 0.f;
            }
            float* e3 = eo + (fr * J + j) * 3;
            e3[0] = ea * k.scale; e3[1] = eb * k.scale; e3[2] = ec * k.scale;
        }
        __syncthreads();
        store_range(a.dst, f0 * J3, J3, (f0 + i) * J3, (f0 + ps.i1) * J3, [&](int fr, int r) { return WINDOW && fr < zh ? 0.f : eo[fr * J3 + r]; });
    }
}

// euler [B, T, J, 3] -> rot6d [B, T, 6J]: R = R_i(a) R_j(b) R_k(c) in closed form.  With (sa, sb, sc) the sines times eps and p(.) the
// place of an axis in the order, R[r][c] = m[p(r)][p(c)] of
//     m = | cb cc             -cb sc              sb    |
//         | sa sb cc + ca sc   ca cc - sa sb sc  -sa cb |
//         | sa sc - ca sb cc   sa cc + ca sb sc   ca cb |
__global__ __launch_bounds__(THREADS) void articulate_rot6d_euler_kernel(const EulArgs k) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Args& a = k.a;
    const int J = k.J, tid = threadIdx.x;
    int* ord = reinterpret_cast<int*>(lds);
    float* buf = lds + EHEAD;
    rot6d_tile(a, J, lds + MAX_J, buf, [&](int n, long long q0) {
        for (int j = tid; j < J; j += THREADS) ord[j] = min(max(k.orders[j], 0), 5);
        __syncthreads();
        for (int q = tid; q < n; q += THREADS) {
            const float* src = a.src + (q0 + q) * 3;
            const Axes o = order_axes(ord[q % J]);
            float sa, ca, sb, cb, sc, cc;
            sincosf(src[0] * k.scale, &sa, &ca);
            sincosf(src[1] * k.scale, &sb, &cb);
            sincosf(src[2] * k.scale, &sc, &cc);
            sa *= o.eps; sb *= o.eps; sc *= o.eps;
            const float m[9] = {cb * cc, -(cb * sc), sb,
                                sa * sb * cc + ca * sc, ca * cc - sa * sb * sc, -(sa * cb),
                                sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb};
            const int p0 = o.i == 0 ? 0 : (o.j == 0 ? 1 : 2), p1 = o.i == 1 ? 0 : (o.j == 1 ? 1 : 2), p2 = o.i == 2 ? 0 : (o.j == 2 ? 1 : 2);
            float* out = buf + 6 * q;
            out[0] = pick9(m, 4 * p0);
            if (k.columns) {
                out[1] = pick9(m, 3 * p1 + p0); out[2] = pick9(m, 3 * p2 + p0);
                out[3] = pick9(m, 3 * p0 + p1); out[4] = pick9(m, 4 * p1); out[5] = pick9(m, 3 * p2 + p1);
            } else {
                out[1] = pick9(m, 3 * p0 + p1); out[2] = pick9(m, 3 * p0 + p2);
                out[3] = pick9(m, 3 * p1 + p0); out[4] = pick9(m, 4 * p1); out[5] = pick9(m, 3 * p1 + p2);
            }
        }
    });
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
                  const float* lengths, int K, const void* d_table, const int32_t* d_frames, int draws, int frame_unit, const void* d_mean) {
    EG_REQUIRE(src, EG_ERR_BAD_ARG, "%s: null input", who);
    EG_REQUIRE(dst, EG_ERR_BAD_ARG, "%s: null output", who);
    EG_REQUIRE(d_table, EG_ERR_BAD_ARG, "%s: null d_table", who);
    int rc = check_table(who, parents, children, lengths, K);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(eg_aligned16(src) && eg_aligned16(dst), EG_ERR_ALIGN, "%s: input / output not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_table) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_mean) & 3u) == 0, EG_ERR_ALIGN,
               "%s: d_table / d_mean not 4-byte aligned", who);
    EG_REQUIRE(B >= 1 && T >= 1, EG_ERR_BAD_ARG, "%s: rows=%d frames=%d (need >= 1)", who, B, T);
    return egi_check_rows(who, B, T, nullptr, d_frames, false, draws, frame_unit, 0, "");
}

// What eg_skeleton_joints and eg_skeleton_rotations check behind their own arguments, in the header's order -- the rate, out_stride, the grid
// and the index range of an output of `per_frame` floats per frame -- and the rest of the kernel's arguments: a.L, a.M, a.tiles, a.T_out.
// `tile`: the output frames of one workgroup.  `window`: the window form, whose out_stride is the output limit, 1 .. t_out, and whose
// a.frames is the [2][rows] table of zero_head.
int forward_args(const char* who, Args& a, int L, int M, long long out_stride, int per_frame, int tile = TF, bool window = false) {
    int rc = reduce_rate(who, L, M);
    if (rc != EG_OK) return rc;
    const long long t_out = out_frames(a.T, L, M);
    if (window) {
        EG_REQUIRE(a.frames, EG_ERR_BAD_ARG, "%s: null d_window (device int32 [2, rows]: valid frames | zeroed head)", who);
        EG_REQUIRE(out_stride >= 1 && out_stride <= t_out, EG_ERR_BAD_ARG, "%s: out_frames=%lld outside 1 .. %lld, the output frames of %d input frames at L=%d / M=%d",
                   who, out_stride, t_out, a.T, L, M);
    } else {
        EG_REQUIRE(out_stride >= t_out, EG_ERR_BAD_ARG, "%s: out_stride=%lld < %lld output frames of %d input frames at L=%d / M=%d", who, out_stride,
                   t_out, a.T, L, M);
    }
    const long long tiles = (out_stride + tile - 1) / tile;
    EG_REQUIRE(tiles * a.B <= 0x7fffffffll && (long long)a.B * out_stride * per_frame < (1ll << 40), EG_ERR_UNSUPPORTED,
               "%s: rows=%d x out_stride=%lld: grid / index range", who, a.B, out_stride);
    a.L = L; a.M = M; a.tiles = (int)tiles; a.T_out = out_stride;
    return EG_OK;
}

// The inverse side's counterpart: the calls at the native rate, whose output has T frames of `per_frame` floats per row.
int inverse_args(const char* who, Args& a, int per_frame, int tile) {
    const long long tiles = ((long long)a.T + tile - 1) / tile;
    EG_REQUIRE(tiles * a.B <= 0x7fffffffll && (long long)a.B * a.T * per_frame < (1ll << 40), EG_ERR_UNSUPPORTED,
               "%s: rows=%d x frames=%d: grid / index range", who, a.B, a.T);
    a.L = 1; a.M = 1; a.tiles = (int)tiles; a.T_out = a.T;
    return EG_OK;
}

// One workgroup per tile of every row.  `a` holds the grid; `k`: what the kernel takes (Args itself, or a block that begins with it).
template <class A>
int launch(void (*kernel)(A), const Args& a, const A& k, size_t lds_floats, void* stream, const char* what) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)a.tiles * a.B)), dim3(THREADS), lds_floats * sizeof(float), static_cast<hipStream_t>(stream), k);
    return eg_check_launch(what);
}
int launch(void (*kernel)(Args), const Args& a, size_t lds_floats, void* stream, const char* what) { return launch(kernel, a, a, lds_floats, stream, what); }

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

namespace {
// Both forms of a forward call share one body: `window` picks the checks of the output limit and the WINDOW instantiation.
int joints_call(const char* who, bool window, const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                const float* lengths, int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                const float* d_mean, int32_t unit, int32_t L, int32_t M, float* joints, int64_t out_stride, void* stream) {
    int rc = common_checks(who, track, joints, rows, T, parents, children, lengths, bones, d_table, d_frames, draws, frame_unit, d_mean);
    if (rc != EG_OK) return rc;
    Args a = {track, static_cast<const int*>(d_table), d_frames, d_mean, joints, rows, T, bones, draws, frame_unit};
    rc = forward_args(who, a, L, M, out_stride, 3 * (bones + 1), TF, window);
    if (rc != EG_OK) return rc;
    const bool native = a.L == 1 && a.M == 1;
    void (*kernel)(Args);
    if (window)
        kernel = unit ? (native ? skeleton_joints_kernel<true, true, true> : skeleton_joints_kernel<true, false, true>)
                      : (native ? skeleton_joints_kernel<false, true, true> : skeleton_joints_kernel<false, false, true>);
    else
        kernel = unit ? (native ? skeleton_joints_kernel<true, true> : skeleton_joints_kernel<true, false>)
                      : (native ? skeleton_joints_kernel<false, true> : skeleton_joints_kernel<false, false>);
    return launch(kernel, a, HEAD + round4(SLOTS * 3 * bones + 8) + (bones + 1) * NC, stream, window ? "skeleton_joints_window" : "skeleton_joints");
}
}  // namespace

extern "C" int eg_skeleton_joints(const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                                  int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                                  const float* d_mean, int32_t unit, int32_t L, int32_t M, float* joints, int64_t out_stride, void* stream) {
    return joints_call("eg_skeleton_joints", false, track, rows, T, parents, children, lengths, bones, d_table, d_frames, draws, frame_unit, d_mean,
                       unit, L, M, joints, out_stride, stream);
}

extern "C" int eg_skeleton_joints_window(const float* window, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                                         const float* lengths, int32_t bones, const void* d_table, const int32_t* d_window, const float* d_mean,
                                         int32_t unit, int32_t L, int32_t M, float* joints, int64_t out_frames, void* stream) {
    return joints_call("eg_skeleton_joints_window", true, window, rows, T, parents, children, lengths, bones, d_table, d_window, 1, 1, d_mean, unit, L,
                       M, joints, out_frames, stream);
}

extern "C" int eg_skeleton_dir_vec(const float* joints, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                                   int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                                   const float* d_mean, float* dir_vec, void* stream) {
    const char* who = "eg_skeleton_dir_vec";
    int rc = common_checks(who, joints, dir_vec, rows, T, parents, children, lengths, bones, d_table, d_frames, draws, frame_unit, d_mean);
    if (rc != EG_OK) return rc;
    Args a = {joints, static_cast<const int*>(d_table), d_frames, d_mean, dir_vec, rows, T, bones, draws, frame_unit};
    rc = inverse_args(who, a, 3 * (bones + 1), TF);
    if (rc != EG_OK) return rc;
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

namespace {
int rotations_call(const char* who, bool window, const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                   const float* lengths, int32_t bones, const double* rest, const void* d_levels, const int32_t* d_frames, int32_t draws,
                   int32_t frame_unit, const float* d_mean, int32_t space, int32_t L, int32_t M, float* rotations, int64_t out_stride, void* stream) {
    int rc = common_checks(who, track, rotations, rows, T, parents, children, lengths, bones, d_levels, d_frames, draws, frame_unit, d_mean);
    if (rc != EG_OK) return rc;
    rc = check_rest(who, rest, bones);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(space == EG_SKELETON_SPACE_LOCAL || space == EG_SKELETON_SPACE_GLOBAL, EG_ERR_BAD_ARG, "%s: space=%d (0: local, 1: global)", who, space);
    Args a = {track, static_cast<const int*>(d_levels), d_frames, d_mean, rotations, rows, T, bones, draws, frame_unit};
    rc = forward_args(who, a, L, M, out_stride, 4 * bones, TF, window);
    if (rc != EG_OK) return rc;
    const bool native = a.L == 1 && a.M == 1, glob = space == EG_SKELETON_SPACE_GLOBAL;
    void (*kernel)(Args);
    if (window)
        kernel = glob ? (native ? skeleton_rotations_kernel<true, true, true> : skeleton_rotations_kernel<false, true, true>)
                      : (native ? skeleton_rotations_kernel<true, false, true> : skeleton_rotations_kernel<false, false, true>);
    else
        kernel = glob ? (native ? skeleton_rotations_kernel<true, true> : skeleton_rotations_kernel<false, true>)
                      : (native ? skeleton_rotations_kernel<true, false> : skeleton_rotations_kernel<false, false>);
    return launch(kernel, a, RHEAD + round4(SLOTS * 3 * bones + 8) + bones * 4 * TF, stream, window ? "skeleton_rotations_window" : "skeleton_rotations");
}
}  // namespace

extern "C" int eg_skeleton_rotations(const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                                     const float* lengths, int32_t bones, const double* rest, const void* d_levels, const int32_t* d_frames,
                                     int32_t draws, int32_t frame_unit, const float* d_mean, int32_t space, int32_t L, int32_t M,
                                     float* rotations, int64_t out_stride, void* stream) {
    return rotations_call("eg_skeleton_rotations", false, track, rows, T, parents, children, lengths, bones, rest, d_levels, d_frames, draws,
                          frame_unit, d_mean, space, L, M, rotations, out_stride, stream);
}

extern "C" int eg_skeleton_rotations_window(const float* window, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                                            const float* lengths, int32_t bones, const double* rest, const void* d_levels, const int32_t* d_window,
                                            const float* d_mean, int32_t space, int32_t L, int32_t M, float* rotations, int64_t out_frames,
                                            void* stream) {
    return rotations_call("eg_skeleton_rotations_window", true, window, rows, T, parents, children, lengths, bones, rest, d_levels, d_window, 1, 1,
                          d_mean, space, L, M, rotations, out_frames, stream);
}

// ---- articulated bodies: host ---------------------------------------------------------------------------------------------------------------
namespace {

int check_body(const char* who, const int32_t* parents, const float* offsets, int J) {
    EG_REQUIRE(parents && offsets, EG_ERR_BAD_ARG, "%s: null parents / offsets", who);
    EG_REQUIRE(J >= 1 && J <= MAX_J, EG_ERR_UNSUPPORTED, "%s: joints=%d (1..%d)", who, J, MAX_J);
    EG_REQUIRE(parents[0] == -1, EG_ERR_BAD_ARG, "%s: joint 0: parent=%d (joint 0 is the root, its parent is -1)", who, parents[0]);
    for (int j = 0; j < J; ++j) {
        EG_REQUIRE(j == 0 || (parents[j] >= 0 && parents[j] < j), EG_ERR_BAD_ARG,
                   "%s: joint %d: parent=%d is not an earlier joint (the table must be in topological order)", who, j, parents[j]);
        const float* o = offsets + 3 * j;
        EG_REQUIRE(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]), EG_ERR_BAD_ARG, "%s: joint %d: offset (%g, %g, %g) is not finite", who, j,
                   (double)o[0], (double)o[1], (double)o[2]);
    }
    return EG_OK;
}

// What both calls check about their rows: the counterpart of common_checks without a bone table.
int rows_checks(const char* who, const void* src, int B, int T, const int32_t* d_frames, int draws, int frame_unit, const void* d_mean, int basis) {
    EG_REQUIRE(src, EG_ERR_BAD_ARG, "%s: null input", who);
    EG_REQUIRE(eg_aligned16(src), EG_ERR_ALIGN, "%s: input not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_mean) & 3u) == 0, EG_ERR_ALIGN, "%s: d_mean not 4-byte aligned", who);
    EG_REQUIRE(B >= 1 && T >= 1, EG_ERR_BAD_ARG, "%s: rows=%d frames=%d (need >= 1)", who, B, T);
    if (int rc = egi_check_rows(who, B, T, nullptr, d_frames, false, draws, frame_unit, 0, "")) return rc;
    EG_REQUIRE(basis == EG_ARTICULATE_BASIS_ROWS || basis == EG_ARTICULATE_BASIS_COLUMNS, EG_ERR_BAD_ARG, "%s: basis=%d (0: rows, 1: columns)", who,
               basis);
    return EG_OK;
}

}  // namespace

extern "C" int eg_articulate_check(const int32_t* parents, const float* offsets, int32_t joints) {
    return check_body("eg_articulate_check", parents, offsets, joints);
}

extern "C" int32_t eg_articulate_tile_frames(void) { return TFA; }

extern "C" int eg_articulate_levels(const int32_t* parents, const float* offsets, int32_t joints, int32_t* words) {
    const char* who = "eg_articulate_levels";
    int rc = check_body(who, parents, offsets, joints);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(words, EG_ERR_BAD_ARG, "%s: null words", who);
    const int J = joints;
    int depth[MAX_J], count[ALEVELS] = {}, at[ALEVELS];
    int nlev = 0;
    for (int j = 0; j < J; ++j) {                       // topological order: the parent came earlier
        depth[j] = j == 0 ? 0 : depth[parents[j]] + 1;
        ++count[depth[j]];
        nlev = depth[j] + 1 > nlev ? depth[j] + 1 : nlev;
    }
    words[0] = nlev;
    for (int l = 0, s = 0; l < ALEVELS; ++l) {
        words[AL_FIRST + l] = s;
        at[l] = s;
        if (l < nlev) s += count[l];
    }
    for (int j = 0; j < J; ++j) words[AL_ORDER + at[depth[j]]++] = j;                  // by depth, table order inside a level
    for (int j = 0; j < J; ++j) words[al_parents(J) + j] = parents[j];
    for (int r = 0; r < 3 * J; ++r) words[al_offsets(J) + r] = *reinterpret_cast<const int32_t*>(offsets + r);
    return EG_OK;
}

namespace {
int articulate_call(const char* who, bool window, const float* track, int32_t rows, int32_t T, const int32_t* parents, const float* offsets,
                    int32_t joints, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean,
                    int32_t basis, int32_t space, int32_t L, int32_t M, float* out_joints, float* out_rotations, int64_t out_stride, void* stream) {
    EG_REQUIRE(out_joints || out_rotations, EG_ERR_BAD_ARG, "%s: null out_joints and out_rotations (need one of them)", who);
    EG_REQUIRE(d_table, EG_ERR_BAD_ARG, "%s: null d_table", who);
    int rc = check_body(who, parents, offsets, joints);
    if (rc != EG_OK) return rc;
    rc = rows_checks(who, track, rows, T, d_frames, draws, frame_unit, d_mean, basis);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(eg_aligned16(out_joints) && eg_aligned16(out_rotations), EG_ERR_ALIGN, "%s: out_joints / out_rotations not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_table) & 3u) == 0, EG_ERR_ALIGN, "%s: d_table not 4-byte aligned", who);
    EG_REQUIRE(space == EG_SKELETON_SPACE_LOCAL || space == EG_SKELETON_SPACE_GLOBAL, EG_ERR_BAD_ARG, "%s: space=%d (0: local, 1: global)", who, space);
    EG_REQUIRE((long long)rows * T * 6 * joints < (1ll << 40), EG_ERR_UNSUPPORTED, "%s: rows=%d x frames=%d: index range", who, rows, T);
    ArtArgs k = {{track, static_cast<const int*>(d_table), d_frames, d_mean, out_joints, rows, T, 2 * joints, draws, frame_unit}, out_rotations, joints,
                 basis == EG_ARTICULATE_BASIS_COLUMNS};
    rc = forward_args(who, k.a, L, M, out_stride, 4 * joints, TFA, window);
    if (rc != EG_OK) return rc;
    const bool native = k.a.L == 1 && k.a.M == 1, glob = space == EG_SKELETON_SPACE_GLOBAL;
    void (*kernel)(ArtArgs);
    if (window)
        kernel = glob ? (native ? articulate_kernel<true, true, true> : articulate_kernel<false, true, true>)
                      : (native ? articulate_kernel<true, false, true> : articulate_kernel<false, false, true>);
    else
        kernel = glob ? (native ? articulate_kernel<true, true> : articulate_kernel<false, true>)
                      : (native ? articulate_kernel<true, false> : articulate_kernel<false, false>);
    return launch(kernel, k.a, k, AHEAD + round4(SLA * 6 * joints + 8) + joints * AST, stream, window ? "articulate_forward_window" : "articulate_forward");
}
}  // namespace

extern "C" int eg_articulate_forward(const float* track, int32_t rows, int32_t T, const int32_t* parents, const float* offsets, int32_t joints,
                                     const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean,
                                     int32_t basis, int32_t space, int32_t L, int32_t M, float* out_joints, float* out_rotations, int64_t out_stride,
                                     void* stream) {
    return articulate_call("eg_articulate_forward", false, track, rows, T, parents, offsets, joints, d_table, d_frames, draws, frame_unit, d_mean,
                           basis, space, L, M, out_joints, out_rotations, out_stride, stream);
}

extern "C" int eg_articulate_forward_window(const float* window, int32_t rows, int32_t T, const int32_t* parents, const float* offsets,
                                            int32_t joints, const void* d_table, const int32_t* d_window, const float* d_mean, int32_t basis,
                                            int32_t space, int32_t L, int32_t M, float* out_joints, float* out_rotations, int64_t out_frames,
                                            void* stream) {
    return articulate_call("eg_articulate_forward_window", true, window, rows, T, parents, offsets, joints, d_table, d_window, 1, 1, d_mean, basis,
                           space, L, M, out_joints, out_rotations, out_frames, stream);
}

extern "C" int eg_articulate_rot6d(const float* quat, int32_t rows, int32_t T, int32_t joints, const int32_t* d_frames, int32_t draws,
                                   int32_t frame_unit, const float* d_mean, int32_t basis, float* rot6d, void* stream) {
    const char* who = "eg_articulate_rot6d";
    EG_REQUIRE(rot6d, EG_ERR_BAD_ARG, "%s: null output", who);
    EG_REQUIRE(joints >= 1 && joints <= MAX_J, EG_ERR_UNSUPPORTED, "%s: joints=%d (1..%d)", who, joints, MAX_J);
    int rc = rows_checks(who, quat, rows, T, d_frames, draws, frame_unit, d_mean, basis);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(eg_aligned16(rot6d), EG_ERR_ALIGN, "%s: output not 16-byte aligned", who);
    ArtArgs k = {{quat, nullptr, d_frames, d_mean, rot6d, rows, T, 2 * joints, draws, frame_unit}, nullptr, joints, basis == EG_ARTICULATE_BASIS_COLUMNS};
    rc = inverse_args(who, k.a, 6 * joints, TFI);
    if (rc != EG_OK) return rc;
    return launch(articulate_rot6d_kernel, k.a, k, 6 * MAX_J + TFI * 6 * joints, stream, "articulate_rot6d");
}

// ---- Euler channels: host -------------------------------------------------------------------------------------------------------------------
namespace {

int check_orders(const char* who, const int32_t* orders, const void* d_orders, int J) {
    EG_REQUIRE(J >= 1 && J <= MAX_J, EG_ERR_UNSUPPORTED, "%s: joints=%d (1..%d)", who, J, MAX_J);
    EG_REQUIRE(orders && d_orders, EG_ERR_BAD_ARG, "%s: null orders / d_orders", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_orders) & 3u) == 0, EG_ERR_ALIGN, "%s: d_orders not 4-byte aligned", who);
    for (int j = 0; j < J; ++j)
        EG_REQUIRE(orders[j] >= 0 && orders[j] <= 5, EG_ERR_BAD_ARG, "%s: joint %d: order code %d (0..5: XYZ XZY YXZ YZX ZXY ZYX)", who, j, orders[j]);
    return EG_OK;
}

}  // namespace

namespace {
int euler_call(const char* who, bool window, const float* track, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
               const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean, int32_t basis, int32_t degrees, int32_t L, int32_t M,
               float* euler, int64_t out_stride, void* stream) {
    EG_REQUIRE(euler, EG_ERR_BAD_ARG, "%s: null output", who);
    int rc = check_orders(who, orders, d_orders, joints);
    if (rc != EG_OK) return rc;
    rc = rows_checks(who, track, rows, T, d_frames, draws, frame_unit, d_mean, basis);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(eg_aligned16(euler), EG_ERR_ALIGN, "%s: output not 16-byte aligned", who);
    EG_REQUIRE((long long)rows * T * 6 * joints < (1ll << 40), EG_ERR_UNSUPPORTED, "%s: rows=%d x frames=%d: index range", who, rows, T);
    EulArgs k = {{track, nullptr, d_frames, d_mean, euler, rows, T, 2 * joints, draws, frame_unit}, static_cast<const int*>(d_orders), joints,
                 basis == EG_ARTICULATE_BASIS_COLUMNS, degrees ? (float)(180.0 / M_PI) : 1.f};
    rc = forward_args(who, k.a, L, M, out_stride, 3 * joints, TFA, window);
    if (rc != EG_OK) return rc;
    const bool native = k.a.L == 1 && k.a.M == 1;
    void (*kernel)(EulArgs);
    if (window) kernel = native ? articulate_euler_kernel<true, true> : articulate_euler_kernel<false, true>;
    else kernel = native ? articulate_euler_kernel<true> : articulate_euler_kernel<false>;
    return launch(kernel, k.a, k, EHEAD + round4(SLA * 6 * joints + 8) + TFA * 3 * joints, stream, window ? "articulate_euler_window" : "articulate_euler");
}
}  // namespace

extern "C" int eg_articulate_euler(const float* track, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
                                   const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean, int32_t basis,
                                   int32_t degrees, int32_t L, int32_t M, float* euler, int64_t out_stride, void* stream) {
    return euler_call("eg_articulate_euler", false, track, rows, T, joints, orders, d_orders, d_frames, draws, frame_unit, d_mean, basis, degrees, L,
                      M, euler, out_stride, stream);
}

extern "C" int eg_articulate_euler_window(const float* window, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
                                          const int32_t* d_window, const float* d_mean, int32_t basis, int32_t degrees, int32_t L, int32_t M,
                                          float* euler, int64_t out_frames, void* stream) {
    return euler_call("eg_articulate_euler_window", true, window, rows, T, joints, orders, d_orders, d_window, 1, 1, d_mean, basis, degrees, L, M,
                      euler, out_frames, stream);
}

extern "C" int eg_articulate_rot6d_euler(const float* euler, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
                                         const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean, int32_t basis,
                                         int32_t degrees, float* rot6d, void* stream) {
    const char* who = "eg_articulate_rot6d_euler";
    EG_REQUIRE(rot6d, EG_ERR_BAD_ARG, "%s: null output", who);
    int rc = check_orders(who, orders, d_orders, joints);
    if (rc != EG_OK) return rc;
    rc = rows_checks(who, euler, rows, T, d_frames, draws, frame_unit, d_mean, basis);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(eg_aligned16(rot6d), EG_ERR_ALIGN, "%s: output not 16-byte aligned", who);
    EulArgs k = {{euler, nullptr, d_frames, d_mean, rot6d, rows, T, 2 * joints, draws, frame_unit}, static_cast<const int*>(d_orders), joints,
                 basis == EG_ARTICULATE_BASIS_COLUMNS, degrees ? (float)(M_PI / 180.0) : 1.f};
    rc = inverse_args(who, k.a, 6 * joints, TFI);
    if (rc != EG_OK) return rc;
    return launch(articulate_rot6d_euler_kernel, k.a, k, EHEAD + TFI * 6 * joints, stream, "articulate_rot6d_euler");
}
