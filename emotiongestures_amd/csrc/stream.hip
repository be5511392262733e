// Streaming synthesis: the device-resident session state (audio ring, prior, per-row counters) and the kernels that advance it.
// The C ABI entries (eg_stream_*, eg_generator_stream_step) live in generator.hip, which knows the generator's geometry and carves the
// state buffer; this file holds the kernels and their launchers.
//
// Counters, int64 [4, U] (ctr[k * U + u]):  k = 0: c, pushes since the row's reset;  1: w, windows done;  2: total, -1 while the row is open,
// else the number of samples the row was fed;  3: ready, what stream_advance_kernel decided for the step after this push (0: no window,
// 1: window 0, 2: window w >= 1, whose head is cross-faded with the prior).
// Ownership: c, total and ready are written by one thread per row in stream_advance_kernel and only read elsewhere; w is written by one
// thread per row in stream_handoff_kernel, where no other thread reads it (they read `ready`).  No atomics, plain stores.
#include "common.h"

namespace {

enum { CTR_C = 0, CTR_W = 1, CTR_TOTAL = 2, CTR_READY = 3 };

inline int stream_grid(size_t n, int cap = 4096) {
    const size_t g = (n + 255) / 256;
    return (int)(g < (size_t)cap ? (g ? g : 1) : cap);
}

// rows selected by mask (all when mask == nullptr): ring zeroed, prior := seed pose, c = w = ready = 0, total = -1
__global__ __launch_bounds__(256) void stream_reset_kernel(float* __restrict__ ring, float* __restrict__ prior, int64_t* __restrict__ ctr,
                                                           const int32_t* __restrict__ mask, const float* __restrict__ seed, int U,
                                                           int64_t ring_len, int PD) {
    const size_t per = (size_t)ring_len + PD, n = (size_t)U * per;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int u = (int)(i / per);
        if (mask && !mask[u]) continue;
        const size_t r = i - (size_t)u * per;
        if (r < (size_t)ring_len) ring[(size_t)u * ring_len + r] = 0.f;
        else prior[(size_t)u * PD + (r - ring_len)] = seed[(size_t)u * PD + (r - ring_len)];
        if (r == 0) {
            ctr[CTR_C * U + u] = 0; ctr[CTR_W * U + u] = 0; ctr[CTR_TOTAL * U + u] = -1; ctr[CTR_READY * U + u] = 0;
        }
    }
}

// one thread per row: c += 1; a row that ends in this push (ends[u] = m in [0, hop]) gets total = (c - 1) * hop + m; then the verdict
// for the step that follows: an open row's window w is ready when c >= w + lag, an ended row's while w * hop < total.
__global__ __launch_bounds__(256) void stream_advance_kernel(int64_t* __restrict__ ctr, const int32_t* __restrict__ ends, int U, int64_t hop,
                                                             int lag) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    const int64_t c = ctr[CTR_C * U + u] + 1, w = ctr[CTR_W * U + u];
    int64_t total = ctr[CTR_TOTAL * U + u];
    if (total < 0 && ends && ends[u] >= 0) total = (c - 1) * hop + (ends[u] < hop ? (int64_t)ends[u] : hop);
    const bool ready = total < 0 ? c >= w + lag : w * hop < total;
    ctr[CTR_C * U + u] = c;
    ctr[CTR_TOTAL * U + u] = total;
    ctr[CTR_READY * U + u] = ready ? (w > 0 ? 2 : 1) : 0;
}

// After stream_advance_kernel.  Items [0, hop) of a row store this push's samples at ring position s mod (lag * hop), s = (c - 1) * hop + j
// the sample's index in the recording (zero from the row's end on); items [hop, hop + n) assemble the row's clip, oldest sample first:
// clip[k] = recording[w * hop + k], with k folded into the window's own L = total - w * hop samples (period 2L, np.pad mode="symmetric")
// once the row has ended -- the rule of window_gather_kernel (misc.hip).  A sample of the newest hop is taken from `chunk`, an older one
// from the ring slots this launch does not write, a sample before the start of the recording (or one the ring no longer holds) is zero;
// a row without a ready window gets an all-zero clip.
__global__ __launch_bounds__(256) void stream_push_kernel(float* __restrict__ ring, const int64_t* __restrict__ ctr,
                                                          const float* __restrict__ chunk, float* __restrict__ clips, int U, int hop,
                                                          int n, int lag) {
    // blockIdx.y walks the rows, so the counters are uniform per workgroup and the per-element arithmetic is 32-bit: the launcher
    // checks lag * hop + n < 2^31.  ring_len = lag * hop, so a push's hop is one contiguous ring slot and nothing wraps inside it.
    const int ring_len = lag * hop, per = hop + n;
    for (int u = blockIdx.y; u < U; u += gridDim.y) {
        const int64_t c = ctr[CTR_C * U + u], total = ctr[CTR_TOTAL * U + u];
        const int64_t newest = (c - 1) * (int64_t)hop, start = ctr[CTR_W * U + u] * (int64_t)hop;
        const bool ready = ctr[CTR_READY * U + u] != 0;
        const int slot_new = (int)((c - 1) % lag) * hop, slot_old = (int)(c % lag) * hop;     // ring positions of samples newest / oldest
        // real samples in this push's chunk (the rest is stored as zero); samples of the window before the fold; where the window starts
        const int real = total < 0 ? hop : (int)(total - newest < 0 ? 0 : (total - newest < hop ? total - newest : hop));
        const int L = (total >= 0 && total - start < n) ? (int)(total - start) : n;               // >= 1 for a ready window
        const int64_t oldest = (c - lag) * (int64_t)hop;
        float* __restrict__ ring_u = ring + (size_t)u * ring_len;
        const float* __restrict__ chunk_u = chunk + (size_t)u * hop;
        for (int64_t r64 = (int64_t)blockIdx.x * 256 + threadIdx.x; r64 < per; r64 += (int64_t)gridDim.x * 256) {     // 64-bit: per may be close to 2^31
            const int r = (int)r64;
            if (r < hop) {
                ring_u[slot_new + r] = r < real ? chunk_u[r] : 0.f;
                continue;
            }
            int k = r - hop;
            float v = 0.f;
            if (ready) {
                if (k >= L) {
                    k = (int)((unsigned)k % (2u * (unsigned)L));
                    if (k >= L) k = (int)(2u * (unsigned)L - 1u - (unsigned)k);        // unsigned: 2L may pass 2^31
                }
                const int64_t s = start + k;
                if (s >= newest) {
                    const int64_t j = s - newest;
                    if (j < real) v = chunk_u[j];
                } else if (s >= 0 && s >= oldest) {
                    int64_t pos = slot_old + (s - oldest);
                    if (pos >= ring_len) pos -= ring_len;
                    v = ring_u[pos];
                }
            }
            clips[(size_t)u * n + (r - hop)] = v;
        }
    }
}

// The stream's hand-off after one generator step at batch U.  pose [U, F, D] is the step's raw output, prior [U, P, D] the state's prior
// (what the step was seeded with), H = F - P.  Per row, from the verdict of the push before it:
//   ready:     rows_out[u, j] = handoff_blend(prior[u, j], pose[u, j]) for j < P when w >= 1, pose[u, j] otherwise (j < H);
//              prior[u, j] := pose[u, H + j];  w += 1;  valid_out[u] = 1;  window_out[u] = pose[u]
//   not ready: rows_out[u] = 0, window_out[u] = 0, valid_out[u] = 0, prior and w untouched.
// The prior is read and overwritten in this one launch at its fixed address: element (u, j, d) belongs to the thread of pose element
// (u, j, d), j < P, which reads it for the blend and then stores the next prior there; no other thread touches it.
__global__ __launch_bounds__(256) void stream_handoff_kernel(const float* __restrict__ pose, float* __restrict__ prior,
                                                             int64_t* __restrict__ ctr, const float* __restrict__ alpha,
                                                             float* __restrict__ rows_out, int32_t* __restrict__ valid_out,
                                                             float* __restrict__ window_out, int U, int F, int P, int D) {
    const int H = F - P;
    const size_t n = (size_t)U * F * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D), j = (int)((i / D) % F), u = (int)(i / ((size_t)D * F));
        const int ready = (int)ctr[CTR_READY * U + u];
        const float v = ready ? pose[i] : 0.f;
        if (window_out) window_out[i] = v;
        float t = v;
        if (j < P && ready) {
            float* p = prior + ((size_t)u * P + j) * D + d;
            if (ready == 2) t = handoff_blend(alpha, j, P, *p, v);
            *p = pose[((size_t)u * F + H + j) * D + d];
        }
        if (j < H) rows_out[((size_t)u * H + j) * D + d] = t;
        if (j == 0 && d == 0) {
            valid_out[u] = ready ? 1 : 0;
            if (ready) ctr[CTR_W * U + u] += 1;
        }
    }
}

}  // namespace

// ---- internal (C++ linkage) launchers used by generator.hip ------------------------------------------------
int egi_stream_reset(float* ring, float* prior, int64_t* ctr, const int32_t* mask, const float* seed, int U, int64_t ring_len, int PD,
                     hipStream_t st) {
    hipLaunchKernelGGL(stream_reset_kernel, dim3(stream_grid((size_t)U * (ring_len + PD))), dim3(256), 0, st, ring, prior, ctr, mask, seed, U,
                       ring_len, PD);
    return eg_check_launch("stream_reset");
}

int egi_stream_push(float* ring, int64_t* ctr, const float* chunk, const int32_t* ends, float* clips, int U, int64_t hop, int n, int lag,
                    hipStream_t st) {
    hipLaunchKernelGGL(stream_advance_kernel, dim3(eg_cdiv(U, 256)), dim3(256), 0, st, ctr, ends, U, hop, lag);
    const int rc = eg_check_launch("stream_advance");
    if (rc) return rc;
    const int gx = stream_grid(((size_t)hop + n + 1) / 2, 1024);       // a grid-stride loop along a row (at least two elements per thread); rows on grid.y
    hipLaunchKernelGGL(stream_push_kernel, dim3(gx, U < 65535 ? U : 65535), dim3(256), 0, st, ring, ctr, chunk, clips, U, (int)hop, n, lag);
    return eg_check_launch("stream_push");
}

int egi_stream_handoff(const float* pose, float* prior, int64_t* ctr, const float* alpha, float* rows_out, int32_t* valid_out,
                       float* window_out, int U, int F, int P, int D, hipStream_t st) {
    hipLaunchKernelGGL(stream_handoff_kernel, dim3(stream_grid((size_t)U * F * D)), dim3(256), 0, st, pose, prior, ctr, alpha, rows_out,
                       valid_out, window_out, U, F, P, D);
    return eg_check_launch("stream_handoff");
}
