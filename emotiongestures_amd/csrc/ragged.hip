// Ragged roll-out (include/emogest.h: eg_generator_forward_rollout_ragged): U recordings with their own window counts W_u in one call.
//   * eg_rollout_ragged_plan: pure host code (no HIP call) -- the working order, the batch of every step and the device table;
//   * rows_by_table_kernel: whole rows moved by an index table (packed recording-major <-> step-major), the ragged stand-in for swap01_kernel;
//   * rollout_handoff_ragged_kernel: the hand-off of one step for its active ranks, and the zero fill of a finished recording's track tail;
//   * window_gather_ragged_kernel: raw audio with per-recording lengths -> packed clips.
// Every output element has exactly one owning thread; nothing here is device-scope.
#include "common.h"
#include <algorithm>
#include <numeric>
#include <vector>

namespace {

inline int grid_for(size_t n, int cap = 4096) {
    const size_t g = (n + 255) / 256;
    return (int)(g < (size_t)cap ? (g ? g : 1) : cap);
}

// gather: out[slot] = in[table[slot]];  scatter: out[table[slot]] = in[slot]  -- rows of `inner` words of type V.  A row is handled by `tpr`
// threads (a power of two <= 256) that read its table entry once and then stride over the row; 256 / tpr rows per workgroup.
template <typename V>
__global__ __launch_bounds__(256) void rows_by_table_kernel(const V* __restrict__ in, V* __restrict__ out, const int32_t* __restrict__ table,
                                                            int rows, unsigned inner, int tpr, int scatter) {
    const int rpb = 256 / tpr, lane = threadIdx.x & (tpr - 1);
    for (long long slot = (long long)blockIdx.x * rpb + threadIdx.x / tpr; slot < rows; slot += (long long)gridDim.x * rpb) {
        const size_t r = (size_t)table[slot];
        const V* src = in + (scatter ? (size_t)slot : r) * inner;
        V* dst = out + (scatter ? r : (size_t)slot) * inner;
        for (unsigned c = lane; c < inner; c += tpr) dst[c] = src[c];
    }
}

// Hand-off after step s for the `active` ranks of that step (a prefix of the working order).  pose [active, F, D] and prior_in / prior_out
// [U, P, D] are indexed by rank; table = slot_row [N] | order [U] | W by rank [U] (eg_rollout_ragged_plan), so rank r is recording
// u = order[r], its packed window row is slot_row[r] + s (slot_row[r] is the recording's offset: slot (0, r)), and it has Wr windows.
//   track [U, T, D], T = Wmax*H + P: rows s*H + j as rollout_handoff_kernel writes them (handoff_blend for j < P and s >= 1);
//   windows [N, F, D] packed recording-major (optional): the raw pose;  prior_out[r] = pose[r, H + j].
// A recording's LAST step (s == Wr - 1) also zeroes its track tail, rows [Wr*H + P, T): thread (j < H, d) owns rows Wr*H + P + k*H + j,
// k < Wmax - Wr, which cover the tail exactly once.
__global__ __launch_bounds__(256) void rollout_handoff_ragged_kernel(const float* __restrict__ pose, const float* __restrict__ prior_in,
                                                                     const float* __restrict__ alpha, float* __restrict__ track,
                                                                     float* __restrict__ windows, float* __restrict__ prior_out,
                                                                     const int32_t* __restrict__ table, int N, int U, int active, int Wmax,
                                                                     int s, int F, int P, int D) {
    const int H = F - P;
    const size_t T = (size_t)Wmax * H + P, n = (size_t)active * F * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D), j = (int)((i / D) % F), r = (int)(i / ((size_t)D * F));
        const int u = table[N + r], Wr = table[N + U + r];
        const float v = pose[i];
        float t = v;
        if (s > 0 && j < P) t = handoff_blend(alpha, j, P, prior_in[((size_t)r * P + j) * D + d], v);
        float* trk = track + (size_t)u * T * D;
        trk[((size_t)s * H + j) * D + d] = t;
        if (windows) windows[(((size_t)table[r] + s) * F + j) * D + d] = v;
        if (j >= H) prior_out[((size_t)r * P + (j - H)) * D + d] = v;
        if (s == Wr - 1 && j < H)
            for (int k = 0; k < Wmax - Wr; ++k) trk[((size_t)(Wr + k) * H + P + j) * D + d] = 0.f;
    }
}

// One workgroup per clip.  meta (int64): lengths [U] | clip offsets [U] (exclusive prefix sum of W_u = ceil(lengths[u] / hop)).  Clip c
// belongs to the last recording u with offsets[u] <= c and is its window w = c - offsets[u]: window_gather_kernel's rule on the
// recording's own L = lengths[u] - w*hop samples.  A table that disagrees with the host's checks (L < 1, length > stride) writes nothing.
__global__ __launch_bounds__(256) void window_gather_ragged_kernel(const float* __restrict__ audio, float* __restrict__ out,
                                                                   const int64_t* __restrict__ meta, int U, int64_t stride, int N, int64_t hop,
                                                                   int n) {
    for (int clip = blockIdx.x; clip < N; clip += gridDim.x) {
        int lo = 0, hi = U - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (meta[U + mid] <= clip) lo = mid; else hi = mid - 1;
        }
        const int64_t len = meta[lo], start = (clip - meta[U + lo]) * hop, L = len - start;
        if (L < 1 || len > stride || start < 0) continue;
        const float* src = audio + (size_t)lo * stride + start;
        for (int i = threadIdx.x; i < n; i += 256) {
            int64_t k = i;
            if (k >= L) {
                k %= 2 * L;
                if (k >= L) k = 2 * L - 1 - k;
            }
            out[(size_t)clip * n + i] = src[k];
        }
    }
}

}  // namespace

// ---- the plan: host only -------------------------------------------------------------------------------------------------------
extern "C" int64_t eg_rollout_ragged_plan_ints(int32_t utterances, int64_t total_windows) {
    if (utterances < 1 || total_windows < utterances || total_windows > (1 << 20)) return 0;
    return total_windows + 2 * (int64_t)utterances;
}

extern "C" int eg_rollout_ragged_plan(const int32_t* windows_per, int32_t U, int32_t* order, int32_t* inverse, int32_t* step_batch,
                                      int32_t* table) {
    EG_REQUIRE(U >= 1, EG_ERR_BAD_ARG, "eg_rollout_ragged_plan: utterances=%d (need >= 1)", U);
    EG_REQUIRE(windows_per, EG_ERR_BAD_ARG, "eg_rollout_ragged_plan: null pointer");
    int64_t N = 0;
    int Wmax = 0;
    for (int u = 0; u < U; ++u) {
        EG_REQUIRE(windows_per[u] >= 1, EG_ERR_BAD_ARG, "eg_rollout_ragged_plan: windows_per[%d]=%d (need >= 1)", u, windows_per[u]);
        N += windows_per[u];
        Wmax = std::max(Wmax, (int)windows_per[u]);
    }
    EG_REQUIRE(N <= (1 << 20), EG_ERR_UNSUPPORTED, "eg_rollout_ragged_plan: total windows=%lld > 2^20", (long long)N);
    std::vector<int32_t> ord(U), off(U);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return windows_per[a] > windows_per[b]; });   // longer first, ties by index
    for (int u = 0, acc = 0; u < U; ++u) { off[u] = acc; acc += windows_per[u]; }
    int slot = 0, active = U;
    for (int s = 0; s < Wmax; ++s) {
        while (active > 0 && windows_per[ord[active - 1]] <= s) --active;      // the active set of a step is a prefix of the order
        if (step_batch) step_batch[s] = active;
        if (table)
            for (int r = 0; r < active; ++r) table[slot + r] = off[ord[r]] + s;
        slot += active;
    }
    for (int r = 0; r < U; ++r) {
        if (order) order[r] = ord[r];
        if (inverse) inverse[ord[r]] = r;
        if (table) { table[N + r] = ord[r]; table[N + U + r] = windows_per[ord[r]]; }
    }
    return EG_OK;
}

// The takes plan (eg_generator_forward_rollout_takes): the ragged plan's table followed by slot_rank [N], the rank of every step-major slot
// (the fusion kernel of draws.hip finds a slot's recording, offset and step through it).
extern "C" int64_t eg_rollout_takes_plan_ints(int32_t utterances, int64_t total_windows) {
    const int64_t ragged = eg_rollout_ragged_plan_ints(utterances, total_windows);
    return ragged > 0 ? ragged + total_windows : 0;
}

extern "C" int eg_rollout_takes_plan(const int32_t* windows_per, int32_t U, int32_t* order, int32_t* inverse, int32_t* step_batch,
                                     int32_t* table) {
    EG_REQUIRE(U >= 1, EG_ERR_BAD_ARG, "eg_rollout_takes_plan: utterances=%d (need >= 1)", U);
    EG_REQUIRE(windows_per, EG_ERR_BAD_ARG, "eg_rollout_takes_plan: null pointer");
    int64_t N = 0;
    int Wmax = 0;
    for (int u = 0; u < U; ++u) {
        EG_REQUIRE(windows_per[u] >= 1, EG_ERR_BAD_ARG, "eg_rollout_takes_plan: windows_per[%d]=%d (need >= 1)", u, windows_per[u]);
        N += windows_per[u];
        Wmax = std::max(Wmax, (int)windows_per[u]);
    }
    EG_REQUIRE(N <= (1 << 20), EG_ERR_UNSUPPORTED, "eg_rollout_takes_plan: total windows=%lld > 2^20", (long long)N);
    std::vector<int32_t> batch(Wmax);
    const int rc = eg_rollout_ragged_plan(windows_per, U, order, inverse, batch.data(), table);
    if (rc) return rc;
    int32_t* slot_rank = table ? table + N + 2 * (int64_t)U : nullptr;
    for (int s = 0, slot = 0; s < Wmax; ++s) {
        if (step_batch) step_batch[s] = batch[s];
        if (slot_rank)
            for (int r = 0; r < batch[s]; ++r) slot_rank[slot + r] = r;
        slot += batch[s];
    }
    return EG_OK;
}

// ---- internal (C++ linkage) launchers used by generator.hip ---------------------------------------------------------------------
int egi_rows_by_table(const void* in, void* out, const int32_t* table, int rows, size_t inner_words, bool scatter, hipStream_t st) {
    const bool wide = (inner_words & 3) == 0 && eg_aligned16(in) && eg_aligned16(out);
    const size_t q = wide ? inner_words / 4 : inner_words;
    int tpr = 1;
    while (tpr < 256 && (size_t)tpr < q) tpr <<= 1;
    const int blocks = grid_for((size_t)rows * tpr);
    if (wide)
        hipLaunchKernelGGL((rows_by_table_kernel<u32x4_t>), dim3(blocks), dim3(256), 0, st, reinterpret_cast<const u32x4_t*>(in),
                           reinterpret_cast<u32x4_t*>(out), table, rows, (unsigned)q, tpr, scatter ? 1 : 0);
    else
        hipLaunchKernelGGL((rows_by_table_kernel<unsigned int>), dim3(blocks), dim3(256), 0, st, reinterpret_cast<const unsigned int*>(in),
                           reinterpret_cast<unsigned int*>(out), table, rows, (unsigned)q, tpr, scatter ? 1 : 0);
    return eg_check_launch("rows_by_table");
}

extern "C" int eg_rows_by_table(const void* in, void* out, const int32_t* d_table, int32_t rows, int64_t row_words, int32_t scatter,
                                void* stream) {
    EG_REQUIRE(in && out && d_table, EG_ERR_BAD_ARG, "eg_rows_by_table: null pointer");
    EG_REQUIRE(rows >= 1 && row_words >= 1 && row_words < ((int64_t)1 << 32), EG_ERR_BAD_ARG, "eg_rows_by_table: rows=%d row_words=%lld", rows,
               (long long)row_words);
    EG_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(d_table)) & 3u) == 0, EG_ERR_ALIGN,
               "eg_rows_by_table: 4-byte alignment");
    return egi_rows_by_table(in, out, d_table, rows, (size_t)row_words, scatter != 0, (hipStream_t)stream);
}

int egi_rollout_handoff_ragged(const float* pose, const float* prior_in, const float* alpha, float* track, float* windows, float* prior_out,
                               const int32_t* table, int N, int U, int active, int Wmax, int s, int F, int P, int D, hipStream_t st) {
    hipLaunchKernelGGL(rollout_handoff_ragged_kernel, dim3(grid_for((size_t)active * F * D)), dim3(256), 0, st, pose, prior_in, alpha, track,
                       windows, prior_out, table, N, U, active, Wmax, s, F, P, D);
    return eg_check_launch("rollout_handoff_ragged");
}

extern "C" int eg_window_gather_ragged(const float* audio, int32_t utterances, int64_t stride, const int64_t* lengths, const int64_t* d_meta,
                                       int64_t hop_samples, int32_t n_samples, float* out, void* stream) {
    EG_REQUIRE(audio && lengths && d_meta && out, EG_ERR_BAD_ARG, "eg_window_gather_ragged: null pointer");
    EG_REQUIRE(utterances >= 1, EG_ERR_BAD_ARG, "eg_window_gather_ragged: utterances=%d (need >= 1)", utterances);
    EG_REQUIRE(stride >= 1 && hop_samples >= 1 && n_samples >= 1, EG_ERR_BAD_ARG, "eg_window_gather_ragged: stride=%lld hop_samples=%lld n_samples=%d",
               (long long)stride, (long long)hop_samples, n_samples);
    int64_t N = 0;
    for (int u = 0; u < utterances; ++u) {
        EG_REQUIRE(lengths[u] >= 1 && lengths[u] <= stride, EG_ERR_BAD_ARG, "eg_window_gather_ragged: lengths[%d]=%lld (need 1 .. stride=%lld)", u,
                   (long long)lengths[u], (long long)stride);
        N += (lengths[u] + hop_samples - 1) / hop_samples;
        EG_REQUIRE(N <= (1 << 20), EG_ERR_UNSUPPORTED, "eg_window_gather_ragged: total windows > 2^20 at recording %d", u);
    }
    hipLaunchKernelGGL(window_gather_ragged_kernel, dim3((unsigned)std::min<int64_t>(N, 65536)), dim3(256), 0, (hipStream_t)stream, audio, out,
                       d_meta, utterances, stride, (int)N, hop_samples, n_samples);
    return eg_check_launch("window_gather_ragged");
}
