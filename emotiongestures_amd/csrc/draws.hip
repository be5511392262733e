// Diverse roll-out (include/emogest.h: eg_generator_forward_rollout_draws): R sampled tracks per recording, the audio tower run once.
//   * draws_fusion_kernel: the fusion input of all U*W*R (clip, draw) rows in ONE pass -- it permutes the caller's [U, R, W] order of
//     `sampled` into draw order, broadcasts a clip's semantic feature over its R draws and adds;
//   * draws_seed_kernel: seed_pose [U, P, D] repeated over the R draws of a recording, the prior of decoder step 0.
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

int egi_draws_seed(const float* seed, float* prior, int U, int R, int PD, hipStream_t st) {
    const size_t n = (size_t)U * R * PD;
    hipLaunchKernelGGL(draws_seed_kernel, dim3(grid_for(n)), dim3(256), 0, st, seed, prior, n, R, PD);
    return eg_check_launch("draws_seed");
}
