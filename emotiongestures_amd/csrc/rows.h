// The rows of a whole-track stage (include/emogest.h, "Rows of whole tracks"): rows = U * draws tracks of T frames; row b belongs to recording
// u = b / draws and has n = clamp(frames[u] * frame_unit, 0, T) valid frames (T without counts).  One home for what every such stage does
// with them: the device count, the exact-span LDS loader, the ascending fold of a row's tile partials, and the host checks.  Internal.
#pragma once
#include "common.h"

// ---- device ------------------------------------------------------------------------------------------------------------------------------------
// Valid frames of recording u.  A stage that refuses short rows passes its `floor`: the host refuses n < floor on its copy of the counts; a
// device count that differs from it reads as 0 -- zeros, nothing out of range.
__device__ __forceinline__ int egi_valid_frames(const int* frames, int u, int frame_unit, int T, int floor = 0) {
    if (!frames) return T;
    const long long v = (long long)frames[u] * frame_unit;
    const int n = (int)(v < 0 ? 0 : (v > T ? T : v));
    return floor > 0 && n < floor ? 0 : n;
}

// Elements [g0, g1) of p -> l, element g at l[g - (g0 & ~3)]; returns the shift g0 & 3.  p is 16-byte aligned, so every 4-element group that
// starts at a multiple of 4 is one aligned 16-byte load; the two ends are scalar loads: nothing outside the span is read.
__device__ __forceinline__ int egi_stage_exact(float* __restrict__ l, const float* __restrict__ p, long long g0, long long g1, int tid, int threads) {
    const long long q0 = g0 & ~3ll;
    for (long long q = q0 + 4 * tid; q < g1; q += 4 * threads) {
        float* d = l + (q - q0);
        if (q >= g0 && q + 4 <= g1) {
            *reinterpret_cast<f4*>(d) = *reinterpret_cast<const f4*>(p + q);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q + e >= g0 && q + e < g1) d[e] = p[q + e];
        }
    }
    return (int)(g0 - q0);
}

// The same span with the same loads, transposed on the way: [g0, g1) is n frames of D columns (g1 - g0 = n * D < 2^31), and column c of frame t
// goes to l[c * pitch + t] -- channel-major, the image a convolution over frames reads with consecutive lanes on consecutive banks.  The
// stores pay for it: the lanes of one store are 4 columns apart, 4 * pitch floats, so give an odd pitch (8 banks, 4-way) and never a
// multiple of 8 (one or two banks).
__device__ __forceinline__ void egi_stage_exact_t(float* __restrict__ l, int pitch, const float* __restrict__ p, long long g0, long long g1, int D,
                                                  int tid, int threads) {
    const long long q0 = g0 & ~3ll;
    for (long long q = q0 + 4 * tid; q < g1; q += 4 * threads) {
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (q >= g0 && q + 4 <= g1) {
            v = *reinterpret_cast<const f4*>(p + q);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q + e >= g0 && q + e < g1) v[e] = p[q + e];
        }
        const int rel = (int)(q - g0);                          // -3 .. : the first group may start before the span
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = rel + e;
            if (i >= 0 && q + e < g1) {
                const int t = i / D;
                l[(i - t * D) * pitch + t] = v[e];
            }
        }
    }
}

// A row's own tiles added in ascending order, sixteen loads in flight (a tile past nt adds +0.0 or 0, which changes no bit).
template <class V>
__device__ __forceinline__ V egi_sum_tiles(const V* __restrict__ src, long long stride, int nt) {
    V acc = 0;
    for (int t = 0; t < nt; t += 16) {
        V v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = t + u < nt ? src[(long long)(t + u) * stride] : 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
    }
    return acc;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------
// The checks of (d_frames, draws, frame_unit) and, for an entry point that takes a host copy of the counts (has_host_counts), of that copy:
// every recording has at least min_frames valid frames.  `why`: the bound as the message words it, the text behind "valid frames < ".  An
// entry point with arguments of its own between the two halves calls twice, first without the host copy.
inline int egi_check_rows(const char* who, int rows, int T, const int32_t* frames, const int32_t* d_frames, bool has_host_counts, int draws,
                          int frame_unit, int min_frames, const char* why) {
    EG_REQUIRE((reinterpret_cast<uintptr_t>(d_frames) & 3u) == 0, EG_ERR_ALIGN, "%s: d_frames not 4-byte aligned", who);
    EG_REQUIRE(draws >= 1 && rows % draws == 0, EG_ERR_BAD_ARG, "%s: rows=%d is not a multiple of draws=%d", who, rows, draws);
    EG_REQUIRE(frame_unit >= 1, EG_ERR_BAD_ARG, "%s: frame_unit=%d (need >= 1)", who, frame_unit);
    if (!has_host_counts) return EG_OK;
    EG_REQUIRE((d_frames == nullptr) == (frames == nullptr), EG_ERR_BAD_ARG,
               "%s: frames (host) and d_frames (device) go together: the counts are checked on the host copy", who);
    if (frames) {
        for (int u = 0; u < rows / draws; ++u) {
            const long long v = (long long)frames[u] * frame_unit, n = v < 0 ? 0 : (v > T ? T : v);
            EG_REQUIRE(n >= min_frames, EG_ERR_BAD_ARG, "%s: recording %d has %lld valid frames < %s", who, u, n, why);
        }
    }
    return EG_OK;
}
