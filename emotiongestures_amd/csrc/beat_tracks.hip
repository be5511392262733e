// Beat-alignment score of whole recordings of any and unequal length, R gesture tracks per recording (eg_beat_align_tracks).
//
// The clip call (mel.hip: eg_beat_align) keeps every per-frame array of a clip in one workgroup's LDS, which caps it at 1024 onset frames.
// Here the per-frame arrays live in the caller's workspace, packed recording after recording at the offsets of the meta table
// (eg_beat_tracks_meta), and every stage whose work grows with the recording is a grid over (tile of 256 frames, recording).  The arithmetic
// that rounds is the clip call's own: beat_stft_frames / beat_gahr are shared (beat_shared.h), the mel bands of a frame are summed ascending
// by one thread, the peak window is an fp32 running sum, the 24 GAHR terms are summed in upstream order; everything else is max / min / OR /
// integer counting, which no order changes.  So a recording that fits the clip call gets the clip call's bits.
//
// Audio half, once per recording (the R draws of a recording read one copy of it):
//   tracks_stft      (frame pair, u)   paired FFT -> mel dB [128][T_u], rms, the pair's dB maximum
//   tracks_dbmax     (u)               max of the pair maxima -> floor = max - 80          (two-level, order-free)
//   tracks_oenv      (tile, u)         flux mean per frame -> oenv, the tile's min / max
//   tracks_norm      (tile, u)         x = (oenv - min) / (max - min + tiny), the tile's "some x != 0" / "a non-finite x" flags
//   tracks_flags     (tile, u)         peak candidates, oenv minima, rms minima per frame
//   tracks_accept    (tile, u)         the wait-suppressed scan as a per-frame rule (below), the tile's count
//   tracks_events    (tile, u)         compaction (tile base = sum of the earlier tiles' counts), both backtracks per event
//   tracks_masks     (event tile, u)   only with audio_beats: multiplicities of the backtracked sets
// Pose half, per (recording, draw) row:
//   tracks_vel       velocity norms of the 8 joint groups -> vel [row][8][Tmax-1]
//   tracks_extrema   (tile, set, row)  argrelextrema(np.less, order, mode clip) per frame of the set's own slice, the tile's count
//   tracks_pbeats    (tile, set, row)  compaction
//   tracks_gahr      (row)             24 lanes walk the ascending lists, lane 0 sums the 24 terms in upstream order
//
// The wait-suppressed scan.  Upstream: n = 0; while n < T: if cand[n]: accept n, n += 2 else n += 1.  Claim: frame t is accepted iff cand[t]
// and t - s is even, s the first frame of the maximal run of consecutive candidates that holds t.
//   (1) The scan lands on every frame whose predecessor is not a candidate (and on frame 0).  The position only moves forward, by 1 or 2,
//       until it passes T, so it lands on t or steps over it; it steps over t only by the += 2 taken at t - 1, which needs cand[t - 1].
//   (2) So it lands on s (s = 0 or cand[s - 1] is false) and accepts it.  By induction over k: having accepted s + 2k it lands next on
//       s + 2k + 2; if that frame is still in the run it is a candidate and is accepted, and s + 2k + 1 was stepped over, never accepted.
//       If it is past the run, the run's frames are exhausted with exactly the even offsets accepted.
//   (3) A frame outside every run is not a candidate and is never accepted.
// The rule needs only cand[] behind t, so one thread per frame evaluates it by walking back to s.  The walk is short: inside a run x does not
// decrease and every frame exceeds the mean of its 9-frame window by delta = 0.07 while x stays in [0, 1]; summing that inequality over a run
// telescopes to a constant, which bounds a run at a few dozen frames.  Correctness does not depend on that bound, only the cost does.
//
// Ownership: every workspace and output element is written by exactly one thread of one launch (the only shared writes are the order-free
// LDS flag ORs the clip kernel uses too).  No device-scope atomics, no fences, no state kept between calls; launches, grids and pointers
// depend on (lengths, frames, draws) only, so a call captures into a hipGraph.
#include "common.h"
#include "beat_shared.h"

#define BT_TILE 256
#define BT_META_HEAD 4          // U, sum T, max T, max frames
#define BT_META_ROW 8           // length, T, frames, offT, t_end, 0, 0, 0

namespace {

struct Rec { int length, T, frames, offT, t_end; };
__device__ __forceinline__ Rec load_rec(const int* __restrict__ meta, int u) {
    const int* r = meta + BT_META_HEAD + u * BT_META_ROW;
    return Rec{r[0], r[1], r[2], r[3], r[4]};
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rank of this thread among the block's flagged threads (thread order) and the block's total; 256 threads, one use per kernel
__device__ __forceinline__ int block_rank(bool f, int& total) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { base += i < w ? wsum[i] : 0; total += wsum[i]; }
    return base + pre;
}

// sum of cnt[0 .. n) over the block (integers: any order)
__device__ __forceinline__ int block_sum_before(const int* __restrict__ cnt, int n) {
    __shared__ int part[4];
    const int tid = threadIdx.x;
    int s = 0;
    for (int i = tid; i < n; i += BT_TILE) s += cnt[i];
    s = wave_sum_i(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void tracks_stft(const float* __restrict__ audio, int stride, const int* __restrict__ meta,
                                                   const float* __restrict__ melfb_t, const float* __restrict__ window,
                                                   const float* __restrict__ twiddle, const int* __restrict__ band, float* __restrict__ meldb,
                                                   float* __restrict__ rms, float* __restrict__ pairmax) {
    __shared__ float redm[4];
    const int u = blockIdx.y, tid = threadIdx.x;
    const Rec r = load_rec(meta, u);
    if ((int)blockIdx.x * 2 >= r.T) return;
    float mx = beat_stft_frames(audio + (size_t)u * stride, r.length, melfb_t, window, twiddle, band, meldb + (size_t)r.offT * 128,
                                rms + r.offT, r.T, blockIdx.x * 2);
    mx = wave_max(mx);
    if ((tid & 63) == 0) redm[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) pairmax[r.offT + blockIdx.x] = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
}

__global__ __launch_bounds__(256) void tracks_dbmax(const int* __restrict__ meta, const float* __restrict__ pairmax,
                                                    float* __restrict__ floor_db) {
    __shared__ float redm[4];
    const int u = blockIdx.x, tid = threadIdx.x;
    const Rec r = load_rec(meta, u);
    const int n = (r.T + 1) / 2;
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 256) mx = fmaxf(mx, pairmax[r.offT + i]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) redm[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) floor_db[u] = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3])) - 80.f;
}

__global__ __launch_bounds__(256) void tracks_oenv(const int* __restrict__ meta, const float* __restrict__ meldb,
                                                   const float* __restrict__ rms, const float* __restrict__ floor_db_u,
                                                   float* __restrict__ oenv, float* __restrict__ tile_lo, float* __restrict__ tile_hi,
                                                   float* __restrict__ oenv_out, float* __restrict__ rms_out) {
    __shared__ float redf[2][4];
    const int u = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * BT_TILE + tid;
    const Rec r = load_rec(meta, u);
    const int T = r.T;
    if ((int)blockIdx.x * BT_TILE >= T) return;
    const float* db = meldb + (size_t)r.offT * 128;
    const float floor_db = floor_db_u[u];
    float lo = INFINITY, hi = -INFINITY;
    if (t < T) {
        float s = 0.f;
        if (t >= 3)
#pragma unroll 8
            for (int m = 0; m < 128; ++m) {
                const float cur = fmaxf(db[(size_t)m * T + t - 2], floor_db), prev = fmaxf(db[(size_t)m * T + t - 3], floor_db);
                s += fmaxf(0.f, cur - prev);
            }
        const float o = s / 128.f;
        oenv[r.offT + t] = o;
        if (oenv_out) oenv_out[r.offT + t] = o;
        if (rms_out) rms_out[r.offT + t] = rms[r.offT + t];
        lo = fminf(lo, o);
        hi = fmaxf(hi, o);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((tid & 63) == 0) { redf[0][tid >> 6] = lo; redf[1][tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        tile_lo[r.offT + blockIdx.x] = fminf(fminf(redf[0][0], redf[0][1]), fminf(redf[0][2], redf[0][3]));
        tile_hi[r.offT + blockIdx.x] = fmaxf(fmaxf(redf[1][0], redf[1][1]), fmaxf(redf[1][2], redf[1][3]));
    }
}

__global__ __launch_bounds__(256) void tracks_norm(const int* __restrict__ meta, const float* __restrict__ oenv,
                                                   const float* __restrict__ tile_lo, const float* __restrict__ tile_hi,
                                                   float* __restrict__ x, int* __restrict__ tile_any) {
    __shared__ float redf[2][4];
    __shared__ int any_s;
    const int u = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * BT_TILE + tid;
    const Rec r = load_rec(meta, u);
    const int T = r.T, tiles = (T + BT_TILE - 1) / BT_TILE;
    if ((int)blockIdx.x >= tiles) return;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = tid; i < tiles; i += 256) { lo = fminf(lo, tile_lo[r.offT + i]); hi = fmaxf(hi, tile_hi[r.offT + i]); }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((tid & 63) == 0) { redf[0][tid >> 6] = lo; redf[1][tid >> 6] = hi; }
    if (tid == 0) any_s = 0;
    __syncthreads();
    lo = fminf(fminf(redf[0][0], redf[0][1]), fminf(redf[0][2], redf[0][3]));
    hi = fmaxf(fmaxf(redf[1][0], redf[1][1]), fmaxf(redf[1][2], redf[1][3]));
    const float den = (hi - lo) + 1.17549435e-38f;
    if (t < T) {
        const float v = (oenv[r.offT + t] - lo) / den;
        x[r.offT + t] = v;
        if (!isfinite(v)) atomicOr(&any_s, 2);      // LDS flags only (order-free): 1 = some x != 0, 2 = a non-finite x
        if (v != 0.f) atomicOr(&any_s, 1);
    }
    __syncthreads();
    if (tid == 0) tile_any[r.offT + blockIdx.x] = any_s;
}

__global__ __launch_bounds__(256) void tracks_flags(const int* __restrict__ meta, const float* __restrict__ oenv,
                                                    const float* __restrict__ rms, const float* __restrict__ x,
                                                    const int* __restrict__ tile_any, uint8_t* __restrict__ cand,
                                                    uint8_t* __restrict__ min_o, uint8_t* __restrict__ min_r, uint8_t* __restrict__ audio_mask,
                                                    int sum_T) {
    __shared__ int any_s;
    const int u = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * BT_TILE + tid;
    const Rec r = load_rec(meta, u);
    const int T = r.T, tiles = (T + BT_TILE - 1) / BT_TILE;
    if ((int)blockIdx.x >= tiles) return;
    if (tid == 0) any_s = 0;
    __syncthreads();
    int any = 0;
    for (int i = tid; i < tiles; i += 256) any |= tile_any[r.offT + i];
    if (any) atomicOr(&any_s, any);
    __syncthreads();
    const bool detect = any_s == 1;
    if (t >= T) return;
    const float* xr = x + r.offT;
    const float* oe = oenv + r.offT;
    const float* rm = rms + r.offT;
    // peak candidates: x[n] == max(x[n-1 : n+1]) and x[n] >= mean(x[n-4 : n+5]) + delta (windows clipped to the recording); fp32, fixed order
    const float v = xr[t];
    const bool is_max = t == 0 || v >= xr[t - 1];
    const int a0 = t - 4 < 0 ? 0 : t - 4, a1 = t + 5 > T ? T : t + 5;
    float s = 0.f;
    for (int i = a0; i < a1; ++i) s += xr[i];
    // peak_pick's numba loop: fp32 running sum, mean and threshold in fp64 with delta cast to fp32 (its guvectorize signature)
    cand[r.offT + t] = detect && is_max && (double)v >= (double)s / (double)(a1 - a0) + (double)0.07f;
    // onset_backtrack minima (frame 0 always): e[i] <= e[i-1] and e[i] < e[i+1]
    min_o[r.offT + t] = t == 0 || (t < T - 1 && oe[t] <= oe[t - 1] && oe[t] < oe[t + 1]);
    min_r[r.offT + t] = t == 0 || (t < T - 1 && rm[t] <= rm[t - 1] && rm[t] < rm[t + 1]);
    if (audio_mask) {                       // the backtracked sets start from zero; tracks_masks writes the frames that carry events
        audio_mask[(size_t)sum_T + r.offT + t] = 0;
        audio_mask[2 * (size_t)sum_T + r.offT + t] = 0;
    }
}

// accepted[t] = cand[t] && (t - start of its run) even; see the proof in the file header
__global__ __launch_bounds__(256) void tracks_accept(const int* __restrict__ meta, const uint8_t* __restrict__ cand,
                                                     uint8_t* __restrict__ accepted, int* __restrict__ tile_cnt,
                                                     uint8_t* __restrict__ audio_mask) {
    const int u = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * BT_TILE + tid;
    const Rec r = load_rec(meta, u);
    if ((int)blockIdx.x * BT_TILE >= r.T) return;
    const uint8_t* c = cand + r.offT;
    bool acc = false;
    if (t < r.T && c[t]) {
        int k = 0;
        while (t - k - 1 >= 0 && c[t - k - 1]) ++k;
        acc = !(k & 1);
    }
    if (t < r.T) {
        accepted[r.offT + t] = acc;
        if (audio_mask) audio_mask[r.offT + t] = acc;      // onset_raw as 0/1
    }
    int total;
    block_rank(acc, total);
    if (tid == 0) tile_cnt[r.offT + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void tracks_events(const int* __restrict__ meta, const uint8_t* __restrict__ accepted,
                                                     const int* __restrict__ tile_cnt, const uint8_t* __restrict__ min_o,
                                                     const uint8_t* __restrict__ min_r, int* __restrict__ ev, int sum_T,
                                                     int* __restrict__ n_ev, int* __restrict__ n_audio_beats) {
    const int u = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * BT_TILE + tid;
    const Rec r = load_rec(meta, u);
    const int tiles = (r.T + BT_TILE - 1) / BT_TILE;
    if ((int)blockIdx.x >= tiles) return;
    const int base = block_sum_before(tile_cnt + r.offT, blockIdx.x);
    const bool acc = t < r.T && accepted[r.offT + t];
    int total;
    const int i = base + block_rank(acc, total);
    if (acc) {                                    // backtrack: the largest minimum <= the event
        ev[r.offT + i] = t;
        int j = t;
        while (!min_o[r.offT + j]) --j;
        ev[(size_t)sum_T + r.offT + i] = j;
        j = t;
        while (!min_r[r.offT + j]) --j;
        ev[2 * (size_t)sum_T + r.offT + i] = j;
    }
    if ((int)blockIdx.x == tiles - 1 && tid == 0) {
        n_ev[u] = base + total;
        if (n_audio_beats) n_audio_beats[u] = base + total;
    }
}

// backtracked sets as multiplicities (two events can share a minimum): the first event of each group of equal frames writes the group's size
__global__ __launch_bounds__(256) void tracks_masks(const int* __restrict__ meta, const int* __restrict__ ev, const int* __restrict__ n_ev,
                                                    int sum_T, uint8_t* __restrict__ audio_mask) {
    const int u = blockIdx.y, i = blockIdx.x * BT_TILE + threadIdx.x;
    const Rec r = load_rec(meta, u);
    const int n = n_ev[u];
    if (i >= n) return;
    for (int a = 1; a < 3; ++a) {
        const int* e = ev + (size_t)a * sum_T + r.offT;
        const int f = e[i];
        if (i > 0 && e[i - 1] == f) continue;
        int c = 1;
        while (i + c < n && e[i + c] == f) ++c;
        audio_mask[(size_t)a * sum_T + r.offT + f] = (uint8_t)min(255, c);
    }
}

// vel = p[t+1] - p[t] on columns 18:42 ++ 150:174, per-group L2 norm summed in numpy's order (no FMA contraction); thread (t, g), g fastest:
// the 8 groups of a frame are two runs of 24 consecutive floats
__global__ __launch_bounds__(256) void tracks_vel(const int* __restrict__ meta, const float* __restrict__ pose, int draws, int Tmax,
                                                  int pose_dim, float* __restrict__ vel) {
    const int row = blockIdx.y, u = row / draws, i = blockIdx.x * BT_TILE + threadIdx.x;
    const Rec r = load_rec(meta, u);
    const int L = r.frames - 1, Lm = Tmax - 1, g = i & 7, t = i >> 3;
    if (t >= L) return;
    const int c0 = g < 4 ? 18 + 6 * g : 150 + 6 * (g - 4);
    const float* r0 = pose + ((size_t)row * Tmax + t) * pose_dim + c0;
    const float* r1 = r0 + pose_dim;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const float d = __fsub_rn(r1[c], r0[c]);
        s = c == 0 ? __fmul_rn(d, d) : __fadd_rn(s, __fmul_rn(d, d));
    }
    vel[((size_t)row * 8 + g) * Lm + t] = __fsqrt_rn(s);
}

// argrelextrema(np.less, order, mode='clip') of returned set q (upstream order: right arm, shoulder, fore arm, wrist, left arm, ...) over the
// set's own slice [s0, s1): right-side curves [t_start*fps : t_end*fps], left-side whole (upstream quirk), both clipped to the recording's L
struct SetSlice { int g, s0, len; };
__device__ __forceinline__ SetSlice set_slice(int q, int L, int r_lo, int r_hi) {
    const int g = q == 0 ? 1 : q == 1 ? 0 : q == 4 ? 5 : q == 5 ? 4 : q;
    const int s0 = q < 4 ? min(r_lo, L) : 0, s1 = q < 4 ? min(r_hi, L) : L;
    return SetSlice{g, s0, s1 > s0 ? s1 - s0 : 0};
}

__global__ __launch_bounds__(256) void tracks_extrema(const int* __restrict__ meta, const float* __restrict__ vel, int draws, int Tmax,
                                                      int fps, int t_start, int order, uint8_t* __restrict__ pflag,
                                                      int* __restrict__ ptile_cnt, uint8_t* __restrict__ pose_mask) {
    const int row = blockIdx.z, q = blockIdx.y, u = row / draws, tid = threadIdx.x, i = blockIdx.x * BT_TILE + tid;
    const Rec r = load_rec(meta, u);
    const int L = r.frames - 1, Lm = Tmax - 1;
    const SetSlice sl = set_slice(q, L, t_start * fps, r.t_end * fps);
    const int len = sl.len;
    const float* c = vel + ((size_t)row * 8 + sl.g) * Lm + sl.s0;
    bool ok = false;
    if (i < len) {
        ok = true;
        for (int k = 1; k <= order && ok; ++k) {
            const int ip = i + k < len ? i + k : len - 1, im_ = i - k > 0 ? i - k : 0;
            ok = c[i] < c[ip] && c[i] < c[im_];
        }
    }
    const size_t o = ((size_t)row * 8 + q) * Lm;
    if (i < Lm) {
        pflag[o + i] = ok;
        if (pose_mask) pose_mask[o + i] = ok;
    }
    int total;
    block_rank(ok, total);
    if (tid == 0) ptile_cnt[((size_t)row * 8 + q) * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void tracks_pbeats(const uint8_t* __restrict__ pflag, const int* __restrict__ ptile_cnt, int Tmax,
                                                     int* __restrict__ pbeat, int* __restrict__ n_pb) {
    const int row = blockIdx.z, q = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * BT_TILE + tid;
    const int Lm = Tmax - 1;
    const size_t o = ((size_t)row * 8 + q) * Lm;
    const int base = block_sum_before(ptile_cnt + ((size_t)row * 8 + q) * gridDim.x, blockIdx.x);
    const bool ok = i < Lm && pflag[o + i];
    int total;
    const int k = base + block_rank(ok, total);
    if (ok) pbeat[o + k] = i;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) n_pb[row * 8 + q] = base + total;
}

// calculate_align: 24 GAHR terms (audio set major), summed in upstream's order, / 24
__global__ __launch_bounds__(64) void tracks_gahr(const int* __restrict__ meta, const int* __restrict__ ev, const int* __restrict__ n_ev,
                                                  int sum_T, const int* __restrict__ pbeat, const int* __restrict__ n_pb, int draws, int Tmax,
                                                  int fps, double sigma, double* __restrict__ score) {
    __shared__ double g24[24];
    const int row = blockIdx.x, u = row / draws, tid = threadIdx.x;
    const Rec r = load_rec(meta, u);
    const int n = n_ev[u], Lm = Tmax - 1;
    if (tid < 24 && n > 0)
        g24[tid] = beat_gahr(ev + (size_t)(tid / 8) * sum_T + r.offT, n, pbeat + ((size_t)row * 8 + tid % 8) * Lm, n_pb[row * 8 + tid % 8], fps,
                             sigma);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < 24; ++i) acc += g24[i];
        score[row] = n > 0 ? acc / 24.0 : (double)NAN;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
struct Shape { int64_t sum_T; int max_T, max_F; };

// The refusals that depend on the shape alone, shared by the meta table, the workspace size and the call.  frames == nullptr: audio half only.
int tracks_shape(const char* who, const int32_t* lengths, const int32_t* frames, int32_t U, int32_t draws, int32_t Tmax, int64_t stride,
                 Shape* out) {
    EG_REQUIRE(lengths, EG_ERR_BAD_ARG, "%s: null lengths", who);
    EG_REQUIRE(U >= 1 && U <= 65535, EG_ERR_BAD_ARG, "%s: U=%d (1..65535 recordings)", who, U);
    Shape s{0, 0, 0};
    for (int u = 0; u < U; ++u) {
        EG_REQUIRE(lengths[u] >= 2048, EG_ERR_BAD_ARG, "%s: lengths[%d]=%d (needs >= 2048)", who, u, lengths[u]);
        EG_REQUIRE(stride < 0 || lengths[u] <= stride, EG_ERR_BAD_ARG, "%s: lengths[%d]=%d exceeds stride=%lld", who, u, lengths[u],
                   (long long)stride);
        const int T = 1 + lengths[u] / 512;
        s.sum_T += T;
        s.max_T = T > s.max_T ? T : s.max_T;
    }
    // packed per-frame offsets are int32 and the mel dB array holds 128 floats per frame
    EG_REQUIRE(s.sum_T <= (1 << 24), EG_ERR_BAD_ARG, "%s: %lld onset frames in all exceed the index range (2^24)", who, (long long)s.sum_T);
    EG_REQUIRE(draws >= 1, EG_ERR_BAD_ARG, "%s: draws=%d (needs >= 1)", who, draws);
    if (frames) {
        EG_REQUIRE(Tmax >= 2, EG_ERR_BAD_ARG, "%s: Tmax=%d (needs >= 2)", who, Tmax);
        for (int u = 0; u < U; ++u) {
            EG_REQUIRE(frames[u] >= 2 && frames[u] <= Tmax, EG_ERR_BAD_ARG, "%s: frames[%d]=%d (2..Tmax=%d)", who, u, frames[u], Tmax);
            s.max_F = frames[u] > s.max_F ? frames[u] : s.max_F;
        }
        EG_REQUIRE((int64_t)U * draws <= 65535, EG_ERR_BAD_ARG, "%s: U*draws=%lld rows exceed the grid range (65535)", who,
                   (long long)U * draws);
        EG_REQUIRE((int64_t)U * draws * 8 * (Tmax - 1) < (1LL << 31), EG_ERR_BAD_ARG,
                   "%s: U*draws*8*(Tmax-1)=%lld pose-beat slots exceed the index range (2^31)", who, (long long)U * draws * 8 * (Tmax - 1));
    }
    *out = s;
    return EG_OK;
}

struct Layout {
    int64_t meldb, rms, pairmax, floor_db, oenv, x, tile_lo, tile_hi, tile_any, tile_cnt, ev, n_ev, cand, min_o, min_r, accepted;
    int64_t vel, pbeat, ptile_cnt, n_pb, pflag, bytes;
    int ptiles;
};
Layout tracks_layout(const Shape& s, int U, int draws, int Tmax, bool with_pose) {
    Layout l{};
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += eg_round_up(bytes, 256); return at; };
    const int64_t ST = s.sum_T;
    l.meldb = take(ST * 128 * 4); l.rms = take(ST * 4); l.pairmax = take(ST * 4); l.floor_db = take((int64_t)U * 4);
    l.oenv = take(ST * 4); l.x = take(ST * 4); l.tile_lo = take(ST * 4); l.tile_hi = take(ST * 4); l.tile_any = take(ST * 4);
    l.tile_cnt = take(ST * 4); l.ev = take(ST * 3 * 4); l.n_ev = take((int64_t)U * 4);
    l.cand = take(ST); l.min_o = take(ST); l.min_r = take(ST); l.accepted = take(ST);
    if (with_pose) {
        const int64_t rows = (int64_t)U * draws, Lm = Tmax - 1;
        l.ptiles = (int)((Lm + BT_TILE - 1) / BT_TILE);
        l.vel = take(rows * 8 * Lm * 4); l.pbeat = take(rows * 8 * Lm * 4); l.ptile_cnt = take(rows * 8 * l.ptiles * 4);
        l.n_pb = take(rows * 8 * 4); l.pflag = take(rows * 8 * Lm);
    }
    l.bytes = o;
    return l;
}

}  // namespace

extern "C" int64_t eg_beat_tracks_meta_ints(int32_t U) { return U >= 1 ? BT_META_HEAD + (int64_t)U * BT_META_ROW : 0; }

extern "C" int eg_beat_tracks_meta(const int32_t* lengths, const int32_t* frames, const int32_t* t_end, int32_t pose_fps, int32_t U,
                                   int32_t* meta) {
    EG_REQUIRE(meta, EG_ERR_BAD_ARG, "eg_beat_tracks_meta: null meta");
    Shape s;
    int mx = 2;
    if (frames && U >= 1)
        for (int u = 0; u < U; ++u) mx = frames[u] > mx ? frames[u] : mx;
    int rc = tracks_shape("eg_beat_tracks_meta", lengths, frames, U, 1, mx, -1, &s);
    if (rc) return rc;
    EG_REQUIRE(!frames || pose_fps > 0, EG_ERR_BAD_ARG, "eg_beat_tracks_meta: pose_fps=%d", pose_fps);
    meta[0] = U; meta[1] = (int32_t)s.sum_T; meta[2] = s.max_T; meta[3] = s.max_F;
    int32_t off = 0;
    for (int u = 0; u < U; ++u) {
        int32_t* r = meta + BT_META_HEAD + u * BT_META_ROW;
        r[0] = lengths[u];
        r[1] = 1 + lengths[u] / 512;
        r[2] = frames ? frames[u] : 0;
        r[3] = off;
        r[4] = !frames ? 0 : t_end ? t_end[u] : frames[u] / pose_fps;
        r[5] = r[6] = r[7] = 0;
        off += r[1];
    }
    return EG_OK;
}

extern "C" int64_t eg_beat_tracks_workspace_bytes(const int32_t* lengths, const int32_t* frames, int32_t U, int32_t draws, int32_t Tmax) {
    Shape s;
    if (tracks_shape("eg_beat_tracks_workspace_bytes", lengths, frames, U, draws, Tmax, -1, &s)) return 0;
    return tracks_layout(s, U, draws, Tmax, frames != nullptr).bytes;
}

extern "C" int eg_beat_align_tracks(const float* audio, int32_t U, int64_t stride, const int32_t* lengths, const int32_t* d_meta,
                                    const float* pose, int32_t draws, int32_t Tmax, int32_t pose_dim, const int32_t* frames, int32_t pose_fps,
                                    int32_t t_start, const int32_t* t_end, double sigma, int32_t order, const float* d_melfb_t,
                                    const float* d_window, const float* d_twiddle, const int32_t* d_band, void* workspace,
                                    int64_t workspace_bytes, double* score, int32_t* n_audio_beats, float* oenv, float* rms,
                                    uint8_t* audio_beats, uint8_t* pose_beats, void* stream) {
    const char* who = "eg_beat_align_tracks";
    EG_REQUIRE(audio && lengths && d_meta && d_melfb_t && d_window && d_twiddle && d_band && workspace, EG_ERR_BAD_ARG, "%s: null pointer", who);
    EG_REQUIRE(!pose || (frames && score), EG_ERR_BAD_ARG, "%s: null frames / score with a pose", who);
    EG_REQUIRE(stride >= 2048 && stride < (1LL << 31), EG_ERR_BAD_ARG, "%s: stride=%lld (2048..2^31-1)", who, (long long)stride);
    Shape s;
    int rc = tracks_shape(who, lengths, pose ? frames : nullptr, U, draws, Tmax, stride, &s);
    if (rc) return rc;
    if (pose) {
        EG_REQUIRE(pose_dim >= 174, EG_ERR_BAD_ARG, "%s: pose_dim=%d (the beat joints are columns 18:42 and 150:174)", who, pose_dim);
        EG_REQUIRE(pose_fps > 0 && order >= 1 && sigma > 0.0, EG_ERR_BAD_ARG, "%s: pose_fps=%d order=%d sigma=%g", who, pose_fps, order, sigma);
        EG_REQUIRE(t_start >= 0 && (int64_t)t_start * pose_fps < (1 << 30), EG_ERR_BAD_ARG, "%s: t_start=%d", who, t_start);
        for (int u = 0; u < U; ++u) {
            const int te = t_end ? t_end[u] : frames[u] / pose_fps;
            EG_REQUIRE(t_start < te && (int64_t)te * pose_fps < (1 << 30), EG_ERR_BAD_ARG, "%s: t_start=%d t_end[%d]=%d", who, t_start, u, te);
        }
    }
    const Layout l = tracks_layout(s, U, draws, Tmax, pose != nullptr);
    EG_REQUIRE(workspace_bytes >= l.bytes, EG_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes,
               (long long)l.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    auto F = [&](int64_t at) { return reinterpret_cast<float*>(ws + at); };
    auto I = [&](int64_t at) { return reinterpret_cast<int*>(ws + at); };
    auto B = [&](int64_t at) { return reinterpret_cast<uint8_t*>(ws + at); };
    const int sum_T = (int)s.sum_T, tiles = eg_cdiv(s.max_T, BT_TILE);
    const dim3 blk(256), gtile(tiles, U);

    hipLaunchKernelGGL(tracks_stft, dim3((s.max_T + 1) / 2, U), blk, 0, st, audio, (int)stride, d_meta, d_melfb_t, d_window, d_twiddle, d_band,
                       F(l.meldb), F(l.rms), F(l.pairmax));
    if ((rc = eg_check_launch("beat_tracks_stft"))) return rc;
    hipLaunchKernelGGL(tracks_dbmax, dim3(U), blk, 0, st, d_meta, F(l.pairmax), F(l.floor_db));
    if ((rc = eg_check_launch("beat_tracks_dbmax"))) return rc;
    hipLaunchKernelGGL(tracks_oenv, gtile, blk, 0, st, d_meta, F(l.meldb), F(l.rms), F(l.floor_db), F(l.oenv), F(l.tile_lo), F(l.tile_hi), oenv,
                       rms);
    if ((rc = eg_check_launch("beat_tracks_oenv"))) return rc;
    hipLaunchKernelGGL(tracks_norm, gtile, blk, 0, st, d_meta, F(l.oenv), F(l.tile_lo), F(l.tile_hi), F(l.x), I(l.tile_any));
    if ((rc = eg_check_launch("beat_tracks_norm"))) return rc;
    hipLaunchKernelGGL(tracks_flags, gtile, blk, 0, st, d_meta, F(l.oenv), F(l.rms), F(l.x), I(l.tile_any), B(l.cand), B(l.min_o), B(l.min_r),
                       audio_beats, sum_T);
    if ((rc = eg_check_launch("beat_tracks_flags"))) return rc;
    hipLaunchKernelGGL(tracks_accept, gtile, blk, 0, st, d_meta, B(l.cand), B(l.accepted), I(l.tile_cnt), audio_beats);
    if ((rc = eg_check_launch("beat_tracks_accept"))) return rc;
    hipLaunchKernelGGL(tracks_events, gtile, blk, 0, st, d_meta, B(l.accepted), I(l.tile_cnt), B(l.min_o), B(l.min_r), I(l.ev), sum_T, I(l.n_ev),
                       n_audio_beats);
    if ((rc = eg_check_launch("beat_tracks_events"))) return rc;
    if (audio_beats) {
        hipLaunchKernelGGL(tracks_masks, dim3(eg_cdiv((s.max_T + 1) / 2, BT_TILE), U), blk, 0, st, d_meta, I(l.ev), I(l.n_ev), sum_T, audio_beats);
        if ((rc = eg_check_launch("beat_tracks_masks"))) return rc;
    }
    if (!pose) return EG_OK;

    const int rows = U * draws;
    hipLaunchKernelGGL(tracks_vel, dim3(eg_cdiv((s.max_F - 1) * 8, BT_TILE), rows), blk, 0, st, d_meta, pose, draws, Tmax, pose_dim, F(l.vel));
    if ((rc = eg_check_launch("beat_tracks_vel"))) return rc;
    const dim3 gp(l.ptiles, 8, rows);
    hipLaunchKernelGGL(tracks_extrema, gp, blk, 0, st, d_meta, F(l.vel), draws, Tmax, pose_fps, t_start, order, B(l.pflag), I(l.ptile_cnt),
                       pose_beats);
    if ((rc = eg_check_launch("beat_tracks_extrema"))) return rc;
    hipLaunchKernelGGL(tracks_pbeats, gp, blk, 0, st, B(l.pflag), I(l.ptile_cnt), Tmax, I(l.pbeat), I(l.n_pb));
    if ((rc = eg_check_launch("beat_tracks_pbeats"))) return rc;
    hipLaunchKernelGGL(tracks_gahr, dim3(rows), dim3(64), 0, st, d_meta, I(l.ev), I(l.n_ev), sum_T, I(l.pbeat), I(l.n_pb), draws, Tmax, pose_fps,
                       sigma, score);
    return eg_check_launch("beat_tracks_gahr");
}

// Test entry: the scan rule and the compaction alone, on a caller-made candidate array.  d_cand [sum T] uint8 (packed as the meta table
// places the recordings) -> events [sum T] int32 (recording u's accepted frames ascending from its offset) and counts [U].  workspace as
// for the audio half (eg_beat_tracks_workspace_bytes with frames == NULL).
extern "C" int eg_beat_tracks_scan(const uint8_t* d_cand, const int32_t* lengths, int32_t U, const int32_t* d_meta, void* workspace,
                                   int64_t workspace_bytes, int32_t* events, int32_t* counts, void* stream) {
    const char* who = "eg_beat_tracks_scan";
    EG_REQUIRE(d_cand && d_meta && workspace && events && counts, EG_ERR_BAD_ARG, "%s: null pointer", who);
    Shape s;
    int rc = tracks_shape(who, lengths, nullptr, U, 1, 0, -1, &s);
    if (rc) return rc;
    const Layout l = tracks_layout(s, U, 1, 0, false);
    EG_REQUIRE(workspace_bytes >= l.bytes, EG_ERR_WORKSPACE, "%s: workspace too small", who);
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    uint8_t* accepted = reinterpret_cast<uint8_t*>(ws + l.accepted);
    uint8_t* every = reinterpret_cast<uint8_t*>(ws + l.min_o);       // "every frame is a minimum": the backtracks are the events themselves
    int* tile_cnt = reinterpret_cast<int*>(ws + l.tile_cnt);
    int* ev = reinterpret_cast<int*>(ws + l.ev);
    const dim3 blk(256), gtile(eg_cdiv(s.max_T, BT_TILE), U);
    EG_HIP_TRY(hipMemsetAsync(every, 1, (size_t)s.sum_T, st), who);
    hipLaunchKernelGGL(tracks_accept, gtile, blk, 0, st, d_meta, d_cand, accepted, tile_cnt, (uint8_t*)nullptr);
    if ((rc = eg_check_launch("beat_tracks_accept"))) return rc;
    hipLaunchKernelGGL(tracks_events, gtile, blk, 0, st, d_meta, accepted, tile_cnt, every, every, ev, (int)s.sum_T, counts, (int*)nullptr);
    if ((rc = eg_check_launch("beat_tracks_events"))) return rc;
    EG_HIP_TRY(hipMemcpyAsync(events, ev, (size_t)s.sum_T * sizeof(int), hipMemcpyDeviceToDevice, st), who);
    return EG_OK;
}
