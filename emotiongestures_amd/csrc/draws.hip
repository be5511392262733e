// Diverse roll-out (include/emogest.h: eg_generator_forward_rollout_draws): R sampled tracks per recording, the audio tower run once.
//   * draws_fusion_kernel: the fusion input of all U*W*R (clip, draw) rows in ONE pass -- it permutes the caller's [U, R, W] order of
//     `sampled` into draw order, broadcasts a clip's semantic feature over its R draws and adds;
//   * draws_seed_kernel: seed_pose [U, P, D] repeated over the R draws of a recording, the prior of decoder step 0.
// Takes (eg_generator_forward_rollout_takes): the same R draws for recordings with their OWN window counts W_u, rows indexed through the
// takes plan's device table slot_row [N] | order [U] | W by rank [U] | slot_rank [N] (ragged.hip: eg_rollout_takes_plan).
//   * takes_fusion_kernel: draws_fusion_kernel with the clip and its draws' rows looked up by slot;
//   * takes_seed_kernel: draws_seed_kernel with the gather into rank order;
//   * takes_handoff_kernel: the ragged hand-off of one step for active*R rows, row rank*R + r.
// Every output element has exactly one owning thread; plain vector stores, no atomics, nothing device-scope.
#include "common.h"

namespace {

// fus_in[(w*U + u)*R + r, q] = sampled[(u*R + r)*W + w, q] + semantic[w*U + u, q], q < Q 16-byte quads of one clip (Q = F*d_model/4).
// A thread owns one quad (n, q) of the semantic feature, n = w*U + u: it is read ONCE into registers and serves the thread's `rc` draws
// r = blockIdx.y*rc ... (the launcher splits R over blockIdx.y only while the x-grid alone would leave the chip idle; semantic is then
// below 8 MiB and its gridDim.y re-reads are served by L2 / Infinity Cache).  The draws loop is unrolled by 4: four independent 16-byte
// loads of `sampled` in flight per lane, then four 16-byte stores.  Every element of `sampled` is read once and every element of fus_in
// written once; lanes of a wave read and write consecutive quads of one row (coalesced, 1 KiB per wave instruction; a wave that
// straddles two clips splits into two runs).  U == 1 or W == 1: the row permutation is the identity, same code.
__global__ __launch_bounds__(256) void draws_fusion_kernel(const f4* __restrict__ sampled, const f4* __restrict__ semantic,
                                                           f4* __restrict__ fus_in, int U, int W, int R, int rc, unsigned Q) {
    const size_t total = (size_t)U * W * Q;
    const int r0 = blockIdx.y * rc, r1 = r0 + rc < R ? r0 + rc : R;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / Q;
        const unsigned q = (unsigned)(i - n * Q);
        const size_t w = n / U, u = n - w * U;
        const f4 sem = semantic[i];
        const f4* src = sampled + ((u * R) * W + w) * Q + q;      // row (u*R + r)*W + w: consecutive draws are W rows apart
        f4* dst = fus_in + (n * R) * Q + q;                       // row n*R + r
        const size_t sstep = (size_t)W * Q;
        int r = r0;
        for (; r + 4 <= r1; r += 4) {
            const f4 a = src[(size_t)r * sstep], b = src[(size_t)(r + 1) * sstep], c = src[(size_t)(r + 2) * sstep],
                     d = src[(size_t)(r + 3) * sstep];
            dst[(size_t)r * Q] = a + sem;
            dst[(size_t)(r + 1) * Q] = b + sem;
            dst[(size_t)(r + 2) * Q] = c + sem;
            dst[(size_t)(r + 3) * Q] = d + sem;
        }
        for (; r < r1; ++r) dst[(size_t)r * Q] = src[(size_t)r * sstep] + sem;
    }
}

// prior[(u*R + r), k] = seed[u, k], k < PD = prior_frames * pose_dim (pose_dim need not be a multiple of 4: scalar accesses; U*R*PD elements)
__global__ __launch_bounds__(256) void draws_seed_kernel(const float* __restrict__ seed, float* __restrict__ prior, size_t n, int R, int PD) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t row = i / PD;
        prior[i] = seed[(row / R) * PD + (i - row * PD)];
    }
}

// fus_in[slot*R + r, q] = sampled[R*off + r*Wr + s, q] + semantic[slot, q] for the step-major slot (s, rank) of recording u = order[rank]:
// off = table[rank] (slot (0, rank) holds the recording's first packed row), Wr = table[N + U + rank], s = table[slot] - off and
// rank = table[N + 2U + slot].  `sampled` [N*R, Q] is in the packed order of the replicated ragged call (recording u*R + r owns the Wr rows
// from R*off + r*Wr), so the row read is below R*off + R*Wr <= N*R.  Otherwise draws_fusion_kernel: a thread owns one quad of the semantic
// feature, reads it once and serves its `rc` draws r = blockIdx.y*rc ... from registers, four independent 16-byte loads in flight before
// the four stores; consecutive draws are Wr rows apart in `sampled` and one row apart in fus_in.
__global__ __launch_bounds__(256) void takes_fusion_kernel(const f4* __restrict__ sampled, const f4* __restrict__ semantic,
                                                           f4* __restrict__ fus_in, const int32_t* __restrict__ table, int N, int U, int R,
                                                           int rc, unsigned Q) {
    const size_t total = (size_t)N * Q;
    const int r0 = blockIdx.y * rc, r1 = r0 + rc < R ? r0 + rc : R;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t slot = i / Q;
        const unsigned q = (unsigned)(i - slot * Q);
        const int rank = table[N + 2 * U + slot];
        const size_t off = (size_t)table[rank], Wr = (size_t)table[N + U + rank], s = (size_t)table[slot] - off;
        const f4 sem = semantic[i];
        const f4* src = sampled + ((size_t)R * off + s) * Q + q;  // row R*off + r*Wr + s
        f4* dst = fus_in + (slot * R) * Q + q;                    // row slot*R + r
        const size_t sstep = Wr * Q;
        int r = r0;
        for (; r + 4 <= r1; r += 4) {
            const f4 a = src[(size_t)r * sstep], b = src[(size_t)(r + 1) * sstep], c = src[(size_t)(r + 2) * sstep],
                     d = src[(size_t)(r + 3) * sstep];
            dst[(size_t)r * Q] = a + sem;
            dst[(size_t)(r + 1) * Q] = b + sem;
            dst[(size_t)(r + 2) * Q] = c + sem;
            dst[(size_t)(r + 3) * Q] = d + sem;
        }
        for (; r < r1; ++r) dst[(size_t)r * Q] = src[(size_t)r * sstep] + sem;
    }
}

// prior[(rank*R + r), k] = seed[order[rank], k], k < PD; n = U*R*PD elements (scalar accesses, as draws_seed_kernel)
__global__ __launch_bounds__(256) void takes_seed_kernel(const float* __restrict__ seed, float* __restrict__ prior,
                                                         const int32_t* __restrict__ order, size_t n, int R, int PD) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t row = i / PD;
        prior[i] = seed[(size_t)order[row / R] * PD + (i - row * PD)];
    }
}

// rollout_handoff_ragged_kernel (ragged.hip) for the active*R rows of step s: row rank*R + r of pose [active*R, F, D] and of prior_in /
// prior_out [U*R, P, D] is draw r of recording u = order[rank] and writes track[u, r] of track [U, R, T, D], T = Wmax*H + P; the optional
// packed windows row is R*off + r*Wr + s (off = table[rank]).  A recording's LAST step (s == Wr - 1) zeroes the tails [Wr*H + P, T) of its R
// tracks: thread (row, j < H, d) owns rows Wr*H + P + k*H + j, k < Wmax - Wr, of its own track, each tail row once per (u, r).
__global__ __launch_bounds__(256) void takes_handoff_kernel(const float* __restrict__ pose, const float* __restrict__ prior_in,
                                                            const float* __restrict__ alpha, float* __restrict__ track,
                                                            float* __restrict__ windows, float* __restrict__ prior_out,
                                                            const int32_t* __restrict__ table, int N, int U, int R, int active, int Wmax,
                                                            int s, int F, int P, int D) {
    const int H = F - P;
    const size_t T = (size_t)Wmax * H + P, n = (size_t)active * R * F * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D), j = (int)((i / D) % F);
        const size_t row = i / ((size_t)D * F);
        const int rank = (int)(row / R), r = (int)(row - (size_t)rank * R);
        const int u = table[N + rank], Wr = table[N + U + rank];
        const float v = pose[i];
        float t = v;
        if (s > 0 && j < P) t = handoff_blend(alpha, j, P, prior_in[(row * P + j) * D + d], v);
        float* trk = track + ((size_t)u * R + r) * T * D;
        trk[((size_t)s * H + j) * D + d] = t;
        if (windows) windows[((((size_t)R * table[rank] + (size_t)r * Wr + s) * F) + j) * D + d] = v;
        if (j >= H) prior_out[(row * P + (j - H)) * D + d] = v;
        if (s == Wr - 1 && j < H)
            for (int k = 0; k < Wmax - Wr; ++k) trk[((size_t)(Wr + k) * H + P + j) * D + d] = 0.f;
    }
}

inline int grid_for(size_t n, int cap = 4096) {
    const size_t g = (n + 255) / 256;
    return (int)(g < (size_t)cap ? (g ? g : 1) : cap);
}

}  // namespace

// ---- internal (C++ linkage) launchers used by generator.hip ------------------------------------------------
// sampled [U, R, W, F*D], semantic [W*U, F*D] (clip order n = w*U + u), fus_in [W*U*R, F*D]; F*D % 4 == 0 and 16-byte aligned pointers
// (the caller checks).  The grid is a function of (U, W, R, F*D) only.
int egi_draws_fusion(const float* sampled, const float* semantic, float* fus_in, int U, int W, int R, size_t clip_floats, hipStream_t st) {
    const unsigned Q = (unsigned)(clip_floats / 4);
    const int gx = grid_for((size_t)U * W * Q);
    // enough workgroups for the chip (256 CUs x 8) from the x-grid alone: every thread takes all R draws; otherwise split R over y
    int gy = (2048 + gx - 1) / gx;
    gy = gy < 1 ? 1 : (gy > R ? R : gy);
    const int rc = (R + gy - 1) / gy;
    gy = (R + rc - 1) / rc;
    hipLaunchKernelGGL(draws_fusion_kernel, dim3(gx, gy), dim3(256), 0, st, reinterpret_cast<const f4*>(sampled),
                       reinterpret_cast<const f4*>(semantic), reinterpret_cast<f4*>(fus_in), U, W, R, rc, Q);
    return eg_check_launch("draws_fusion");
}

// sampled [N*R, F*D] in the replicated ragged call's packed order, semantic [N, F*D] in step-major slot order, fus_in [N*R, F*D], table: the
// takes plan on the device [2N + 2U]; alignment as egi_draws_fusion.  The grid is a function of (N, R, F*D) only.
int egi_takes_fusion(const float* sampled, const float* semantic, float* fus_in, const int32_t* table, int N, int U, int R, size_t clip_floats,
                     hipStream_t st) {
    const unsigned Q = (unsigned)(clip_floats / 4);
    const int gx = grid_for((size_t)N * Q);
    int gy = (2048 + gx - 1) / gx;              // egi_draws_fusion's rule: split R over y only while the x-grid alone leaves the chip idle
    gy = gy < 1 ? 1 : (gy > R ? R : gy);
    const int rc = (R + gy - 1) / gy;
    gy = (R + rc - 1) / rc;
    hipLaunchKernelGGL(takes_fusion_kernel, dim3(gx, gy), dim3(256), 0, st, reinterpret_cast<const f4*>(sampled),
                       reinterpret_cast<const f4*>(semantic), reinterpret_cast<f4*>(fus_in), table, N, U, R, rc, Q);
    return eg_check_launch("takes_fusion");
}

// order: the plan's rank -> recording section on the device
int egi_takes_seed(const float* seed, float* prior, const int32_t* order, int U, int R, int PD, hipStream_t st) {
    const size_t n = (size_t)U * R * PD;
    hipLaunchKernelGGL(takes_seed_kernel, dim3(grid_for(n)), dim3(256), 0, st, seed, prior, order, n, R, PD);
    return eg_check_launch("takes_seed");
}

int egi_takes_handoff(const float* pose, const float* prior_in, const float* alpha, float* track, float* windows, float* prior_out,
                      const int32_t* table, int N, int U, int R, int active, int Wmax, int s, int F, int P, int D, hipStream_t st) {
    hipLaunchKernelGGL(takes_handoff_kernel, dim3(grid_for((size_t)active * R * F * D)), dim3(256), 0, st, pose, prior_in, alpha, track,
                       windows, prior_out, table, N, U, R, active, Wmax, s, F, P, D);
    return eg_check_launch("takes_handoff");
}

int egi_draws_seed(const float* seed, float* prior, int U, int R, int PD, hipStream_t st) {
    const size_t n = (size_t)U * R * PD;
    hipLaunchKernelGGL(draws_seed_kernel, dim3(grid_for(n)), dim3(256), 0, st, seed, prior, n, R, PD);
    return eg_check_launch("draws_seed");
}
