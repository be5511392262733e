// The delay line of a stream's delayed output stage (include/emogest.h: eg_render_stream_*; emotiongestures_amd/render.py).  A stream emits H
// pose frames per step; its smoothed joints at a renderer's frame rate need frames that lie behind the step (the filter's half window) and one
// frame ahead of an output (the interpolator's look-ahead).  Let the output run d source frames behind the rows just emitted and both fit: with
// y the smoothed track (smooth.hip's stream output, `half` frames behind; or the raw track, half = 0), step s makes its outputs from the window
//     y[sH - d .. sH - d + W),   W = H + 1 where the rate changes, else H,
// which is [history (delta = d - half frames) | chunk[0 .. W - delta)]: the chunk starts at frame sH - half.  This file keeps that history.
//   state    history [rows][delta][D] fp32 | count [rows] int32 (valid steps so far)
//   push     window [rows][W][D] = history | chunk, for the valid rows, and the table the window form of the output kernels reads
//            (skeleton.hip: zero_head): d_window int32 [2][rows] = the window's valid frames (W, or 0 for a row that is not valid) | its zeroed
//            head (`lead` output frames in a row's first valid step -- the frames before frame 0 of the track --, else 0).  Then the new history,
//            the chunk's last delta frames, and the count in a launch of their own, so that no launch reads and overwrites the state.
//   tail     window [rows][delta + F][D] = history | last, `last` the track's last F frames (the smoother's tail, or the raw tail); a row
//            without a valid step has no track: 0 valid frames.  The state is read only.
// Nothing here depends on the step index: one captured graph replays it.  A copy with one owning thread per element of the window: a thread owns
// an aligned quad of the window and writes it with one 16-byte store where the quad lies inside one valid row, else float by float; it loads 16
// bytes where the four floats come from one source and lie on a 16-byte boundary there, else float by float -- D and delta * D are no multiples
// of 4 (126, 282), so the rows of the window, of the chunk and of the history each start on any float.  No atomics, no memset.
#include "rows.h"

namespace {

struct RArgs {
    float* hist;                                        // [rows][delta][D]
    int* count;                                         // [rows]
    const float* src;                                   // push: chunk [rows][H][D]; tail: last [rows][F][D]
    const int* valid;                                   // push: device int32 [rows] or null (all valid); reset: the row mask
    float* window;                                      // [rows][W][D]
    int* meta;                                          // [2][rows]
    int rows, S, D, delta, W, lead;                     // S: frames of a row of src
};

// TAIL: a row is valid when it has emitted a step, and its head is 0.
template <bool TAIL>
__global__ __launch_bounds__(256) void render_window_kernel(const RArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int WD = a.W * a.D, dD = a.delta * a.D, SD = a.S * a.D;
    const long long total = (long long)a.rows * WD;
    auto is_valid = [&](int u) { return TAIL ? a.count[u] > 0 : (!a.valid || a.valid[u] != 0); };
    if (t < a.rows) {                                   // the table of the output launches: one thread per row
        const int u = (int)t;
        const bool v = is_valid(u);
        a.meta[u] = v ? a.W : 0;
        a.meta[a.rows + u] = (!TAIL && v && a.count[u] == 0) ? a.lead : 0;
    }
    const long long q = 4 * t;                          // this thread's quad of the window
    if (q >= total) return;
    const int u = (int)(q / WD), r = (int)(q - (long long)u * WD);
    if (r + 4 <= WD && q + 4 <= total) {                // inside one row
        if (!is_valid(u)) return;
        const bool from_hist = r + 4 <= dD, from_src = r >= dD;
        const float* s = from_hist ? a.hist + (long long)u * dD + r : a.src + (long long)u * SD + (r - dD);
        f4 v;
        if ((from_hist || from_src) && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
            v = *reinterpret_cast<const f4*>(s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int re = r + e;
                v[e] = re < dD ? a.hist[(long long)u * dD + re] : a.src[(long long)u * SD + (re - dD)];
            }
        }
        *reinterpret_cast<f4*>(a.window + q) = v;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                       // a quad that straddles two rows, or the last one
        const long long g = q + e;
        if (g >= total) break;
        const int ue = (int)(g / WD), re = (int)(g - (long long)ue * WD);
        if (is_valid(ue)) a.window[g] = re < dD ? a.hist[(long long)ue * dD + re] : a.src[(long long)ue * SD + (re - dD)];
    }
}

// The new history (the last delta frames of the chunk: delta <= H) and the count, for the valid rows.
__global__ __launch_bounds__(256) void render_state_kernel(const RArgs a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int dD = a.delta * a.D;
    if (e < a.rows && (!a.valid || a.valid[e] != 0)) a.count[e] += 1;
    if (e >= (long long)a.rows * dD) return;
    const int u = (int)(e / dD), rem = (int)(e - (long long)u * dD);
    if (a.valid && a.valid[u] == 0) return;
    a.hist[e] = a.src[((long long)u * a.S + (a.S - a.delta)) * a.D + rem];
}

__global__ __launch_bounds__(256) void render_reset_kernel(const RArgs a) {           // a.valid: the row mask
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int dD = a.delta * a.D;
    if (e < a.rows && (!a.valid || a.valid[e] != 0)) a.count[e] = 0;
    if (e >= (long long)a.rows * dD) return;
    const int u = (int)(e / dD);
    if (a.valid && a.valid[u] == 0) return;
    a.hist[e] = 0.f;
}

int state_checks(const char* who, const void* state, int rows, int D, int delta) {
    EG_REQUIRE(state, EG_ERR_BAD_ARG, "%s: null state", who);
    EG_REQUIRE(eg_aligned16(state), EG_ERR_ALIGN, "%s: state not 16-byte aligned", who);
    EG_REQUIRE(rows >= 1 && D >= 1, EG_ERR_BAD_ARG, "%s: rows=%d D=%d (need >= 1)", who, rows, D);
    EG_REQUIRE(delta >= 0 && delta <= EG_RENDER_STREAM_MAX_DELTA, EG_ERR_BAD_ARG, "%s: delta=%d (0..%d frames of history)", who, delta,
               EG_RENDER_STREAM_MAX_DELTA);
    EG_REQUIRE((long long)rows * (delta + 1) * D < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: rows=%d x delta=%d x D=%d: index range", who, rows, delta, D);
    return EG_OK;
}

RArgs args_of(void* state, int rows, int S, int D, int delta, int W, int lead, const float* src, const int* valid, float* window, int* meta) {
    float* hist = static_cast<float*>(state);
    return {hist, reinterpret_cast<int*>(hist + (long long)rows * delta * D), src, valid, window, meta, rows, S, D, delta, W, lead};
}

int launch_threads(void (*kernel)(RArgs), const RArgs& a, long long threads, void* stream, const char* what) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return eg_check_launch(what);
}

long long max_ll(long long x, long long y) { return x > y ? x : y; }

}  // namespace

extern "C" int64_t eg_render_stream_state_bytes(int32_t rows, int32_t D, int32_t delta) {
    if (rows < 1 || D < 1 || delta < 0 || delta > EG_RENDER_STREAM_MAX_DELTA) {
        eg_set_error("eg_render_stream_state_bytes: rows=%d D=%d delta=%d (rows, D >= 1; delta 0..%d)", rows, D, delta, EG_RENDER_STREAM_MAX_DELTA);
        return 0;
    }
    return 4ll * ((long long)rows * delta * D + rows);
}

extern "C" int eg_render_stream_reset(void* state, int32_t rows, int32_t D, int32_t delta, const int32_t* row_mask, void* stream) {
    const char* who = "eg_render_stream_reset";
    int rc = state_checks(who, state, rows, D, delta);
    if (rc != EG_OK) return rc;
    const RArgs a = args_of(state, rows, 0, D, delta, 0, 0, nullptr, row_mask, nullptr, nullptr);
    return launch_threads(render_reset_kernel, a, max_ll((long long)rows * delta * D, rows), stream, "render_stream_reset");
}

extern "C" int eg_render_stream_push(void* state, int32_t rows, int32_t H, int32_t D, int32_t delta, int32_t frames, int32_t lead,
                                     const float* chunk, const int32_t* d_valid, float* window, int32_t* d_window, void* stream) {
    const char* who = "eg_render_stream_push";
    int rc = state_checks(who, state, rows, D, delta);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(chunk && window && d_window, EG_ERR_BAD_ARG, "%s: null chunk / window / d_window", who);
    EG_REQUIRE(eg_aligned16(window) && eg_aligned16(chunk), EG_ERR_ALIGN, "%s: chunk / window not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_window) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_valid) & 3u) == 0, EG_ERR_ALIGN,
               "%s: d_window / d_valid not 4-byte aligned", who);
    EG_REQUIRE(H >= 1 && delta <= H, EG_ERR_BAD_ARG, "%s: delta=%d > H=%d frames per step (the new history is the chunk's last delta frames)", who,
               delta, H);
    EG_REQUIRE(frames > delta && frames - delta <= H, EG_ERR_BAD_ARG, "%s: frames=%d: a window is delta=%d frames of history and 1..H=%d of the chunk",
               who, frames, delta, H);
    EG_REQUIRE(lead >= 0, EG_ERR_BAD_ARG, "%s: lead=%d (need >= 0)", who, lead);
    EG_REQUIRE((long long)rows * (H + delta + 1) * D < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: rows=%d x H=%d x D=%d: index range", who, rows, H, D);
    const RArgs a = args_of(state, rows, H, D, delta, frames, lead, chunk, d_valid, window, d_window);
    rc = launch_threads(render_window_kernel<false>, a, max_ll(((long long)rows * frames * D + 3) / 4, rows), stream, "render_stream_push");
    if (rc != EG_OK) return rc;
    return launch_threads(render_state_kernel, a, max_ll((long long)rows * delta * D, rows), stream, "render_stream_state");
}

extern "C" int eg_render_stream_tail(const void* state, int32_t rows, int32_t F, int32_t D, int32_t delta, const float* last, float* window,
                                     int32_t* d_window, void* stream) {
    const char* who = "eg_render_stream_tail";
    int rc = state_checks(who, state, rows, D, delta);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(last && window && d_window, EG_ERR_BAD_ARG, "%s: null last / window / d_window", who);
    EG_REQUIRE(eg_aligned16(window) && eg_aligned16(last), EG_ERR_ALIGN, "%s: last / window not 16-byte aligned", who);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_window) & 3u) == 0, EG_ERR_ALIGN, "%s: d_window not 4-byte aligned", who);
    EG_REQUIRE(F >= 1, EG_ERR_BAD_ARG, "%s: F=%d last frames (need >= 1)", who, F);
    EG_REQUIRE((long long)rows * (F + delta) * D < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: rows=%d x F=%d x D=%d: index range", who, rows, F, D);
    const RArgs a = args_of(const_cast<void*>(state), rows, F, D, delta, F + delta, 0, last, nullptr, window, d_window);
    return launch_threads(render_window_kernel<true>, a, max_ll(((long long)rows * (F + delta) * D + 3) / 4, rows), stream, "render_stream_tail");
}
