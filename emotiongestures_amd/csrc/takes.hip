// Take diversity of whole tracks (include/emogest.h: eg_take_meta, eg_track_rows_pack, eg_take_distance).
//   * track_rows_pack_kernel: the valid rows of track [U, R, Tmax, D] into packed order [N, Dpad] (recording-major, then draw, then frame),
//     pad columns zero: the input of the FGD encoder's first product, with no concatenation and no padded rows;
//   * take_distance_kernel: fp64 sum of squared differences of every pair of takes over one chunk of EG_TAKE_CHUNK_FRAMES frames ->
//     workspace[chunk slot, pair];
//   * take_finish_kernel: chunk partials in ascending order -> scale -> sqrt -> distance [U, R, R] and diversity [U].
// Every output element has exactly one owning thread; plain vector stores, no atomics, nothing device-scope.  The second launch reads what
// the first wrote: the kernel boundary on one stream is the only ordering used.
#include "common.h"

namespace {

constexpr int CH = EG_TAKE_CHUNK_FRAMES;
constexpr int MAXR = EG_TAKE_MAX_DRAWS;
constexpr int REG_QUADS = 8;                            // 16-byte quads of take r's chunk a thread keeps: 256 threads * 8 * 4 floats = CH * 512
constexpr int MAX_U = 65535;                            // blockIdx.y carries the recording

// The chunk slots of recording u start at off[u] / CH + u: floor((off + f) / CH) + 1 >= floor(off / CH) + ceil(f / CH), so the slots of
// consecutive recordings never overlap and the table needs nothing beyond `frames | off`; at most U slots stay unused (never written, never read).
__host__ __device__ inline long long slot_base(int off, int u) { return (long long)(off / CH) + u; }
__host__ __device__ inline int pair_base(int r, int R) { return r * (2 * R - r - 1) / 2; }      // index of pair (r, r + 1) in lexicographic order

// rows[(R*off[u] + r*f + t), :] = track[u, r, t, :] | 0.  blockIdx.y = u; the x-grid strides over the R*f*Q quads of that recording.
// IT: index type of the recording-local quad counter (32-bit where R*f*Q fits: one 32-bit division per quad instead of a 64-bit one).
template <bool VEC, typename IT>
__global__ __launch_bounds__(256) void track_rows_pack_kernel(const float* __restrict__ track, const int* __restrict__ meta,
                                                              f4* __restrict__ rows, int U, int R, int Tmax, int D, int Q) {
    const int u = blockIdx.y;
    const int f = meta[u], off = meta[U + u];
    const IT total = (IT)R * (IT)f * (IT)Q;
    const float* src_u = track + (size_t)u * R * Tmax * D;
    f4* dst_u = rows + (size_t)R * off * Q;
    for (IT i = (IT)blockIdx.x * 256 + threadIdx.x; i < total; i += (IT)gridDim.x * 256) {
        const IT row = i / (IT)Q;
        const int q = (int)(i - row * (IT)Q);
        const IT r = row / (IT)f, t = row - r * (IT)f;
        const float* src = src_u + ((size_t)r * Tmax + (size_t)t) * D + 4 * q;
        f4 v;
        if (VEC) {
            v = *reinterpret_cast<const f4*>(src);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 4 * q + e < D ? src[e] : 0.f;
        }
        dst_u[(size_t)i] = v;                                   // packed rows of one recording are contiguous: quad i of the recording
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {      // xor butterfly: a fixed order, the same value in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Four running sums per thread, one per column of the quad (independent fma chains), folded as (0 + 1) + (2 + 3) before the lane reduction.
struct Acc4 { double s[4]; };
__device__ __forceinline__ void sqdiff4(const f4& a, const f4& b, Acc4& acc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double d = (double)a[e] - (double)b[e];           // each fp32 operand widened before the subtraction
        acc.s[e] = fma(d, d, acc.s[e]);
    }
}

// blockIdx.y = u, blockIdx.x -> logical id chunk * (R - 1) + r (XCD-aware order, below).  The workgroup owns pairs (r, r') for r' > r over frames [chunk*CH, chunk*CH + nf) of
// recording u.  A take's chunk is nf*K contiguous floats; thread `tid` takes quads tid, tid + 256, ... of it, in that order, for every take, so
// a pair's per-thread sum has one order whatever the grid.  REG (K <= 512): take r's quads stay in registers over the r' loop and every
// other take's chunk is read once per base take below it (R - 1 reads in all, L2-served after the first: a 16-frame chunk of 32 takes is 1 MiB
// against 4 MiB of L2 per XCD).  Registers, not LDS, for take r: staging it in LDS and re-reading it per pair measured 13-23 % slower
// (DESIGN.md §10).  !REG: wider rows, both operands re-read per pair.
template <bool REG>
__global__ __launch_bounds__(256) void take_distance_kernel(const f4* __restrict__ feat, const int* __restrict__ meta, double* __restrict__ ws,
                                                            int U, int R, int Kq) {
    const int u = blockIdx.y;
    const int f = meta[u], off = meta[U + u];
    const int tiles = R - 1;
    // Workgroups are dealt round-robin to the 8 XCDs in launch order, so x and x + 8 share an L2.  Give each residue class of x a contiguous
    // run of logical ids: the R - 1 workgroups of one chunk then mostly share an XCD and the re-reads of the chunk hit its L2 (placement is
    // for speed only; every logical id is taken exactly once whatever the hardware does).
    const int gx = gridDim.x, xcd = blockIdx.x & 7, q8 = gx >> 3, r8 = gx & 7;
    const int log = xcd * q8 + (xcd < r8 ? xcd : r8) + (blockIdx.x >> 3);
    const int c = log / tiles, r = log - c * tiles;
    const int t0 = c * CH;
    if (t0 >= f) return;                                        // workgroup-uniform: a shorter recording than the grid's longest
    const int nf = f - t0 < CH ? f - t0 : CH;
    const unsigned nq = (unsigned)nf * (unsigned)Kq;            // quads of one take's chunk
    const size_t take_q = (size_t)f * Kq;                       // quads of one whole take
    const f4* base = feat + ((size_t)R * off + t0) * Kq;        // take 0's chunk
    const f4* pa = base + (size_t)r * take_q;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double red[MAXR][4];

    f4 a[REG ? REG_QUADS : 1];
    if (REG) {
#pragma unroll
        for (int j = 0; j < REG_QUADS; ++j) {
            const unsigned q = (unsigned)j * 256u + tid;
            a[j] = q < nq ? pa[q] : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
    for (int rp = r + 1; rp < R; ++rp) {
        const f4* pb = base + (size_t)rp * take_q;
        Acc4 acc4 = {{0.0, 0.0, 0.0, 0.0}};
        if (REG) {
#pragma unroll
            for (int j = 0; j < REG_QUADS; ++j) {
                const unsigned q = (unsigned)j * 256u + tid;
                const f4 b = q < nq ? pb[q] : f4{0.f, 0.f, 0.f, 0.f};       // past the chunk: 0 - 0, adds +0.0
                sqdiff4(a[j], b, acc4);
            }
        } else {
            for (unsigned q = tid; q < nq; q += 256u) sqdiff4(pa[q], pb[q], acc4);
        }
        const double acc = wave_sum_f64((acc4.s[0] + acc4.s[1]) + (acc4.s[2] + acc4.s[3]));
        if (lane == 0) red[rp - r - 1][wave] = acc;
    }
    __syncthreads();
    const int np = R - 1 - r;
    if (tid < np) {                                             // one thread per pair: waves 0..3 in order, one plain store
        const double s = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
        const int P = R * (R - 1) / 2;
        ws[(size_t)(slot_base(off, u) + c) * P + pair_base(r, R) + tid] = s;
    }
}

// One workgroup per recording.  Thread p (stride 256) sums pair p's chunk partials in ascending chunk order (8 independent loads in flight,
// added in order), scales, takes the root and writes both triangles; then thread 0 sums the pairs in lexicographic order.
__global__ __launch_bounds__(256) void take_finish_kernel(const double* __restrict__ ws, const int* __restrict__ meta, double* __restrict__ dist,
                                                          double* __restrict__ div, int U, int R, int span) {
    const int u = blockIdx.x;
    const int f = meta[u], off = meta[U + u];
    const int P = R * (R - 1) / 2;
    const int nch = (f + CH - 1) / CH;
    const double scale = span > 0 ? (double)span / (double)f : 1.0;
    const double* w0 = ws + (size_t)slot_base(off, u) * P;
    double* d_u = dist + (size_t)u * R * R;
    __shared__ double dl[MAXR * (MAXR - 1) / 2];
    for (int p = threadIdx.x; p < P; p += 256) {
        const double* w = w0 + p;
        double s = 0.0;
        int c = 0;
        for (; c + 8 <= nch; c += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = w[(size_t)(c + k) * P];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; c < nch; ++c) s += w[(size_t)c * P];
        const double d = sqrt(s * scale);
        int r = 0, rem = p;
        while (rem >= R - 1 - r) { rem -= R - 1 - r; ++r; }
        const int rp = r + 1 + rem;
        d_u[r * R + rp] = d;
        d_u[rp * R + r] = d;
        dl[p] = d;
    }
    for (int r = threadIdx.x; r < R; r += 256) d_u[r * R + r] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += dl[p];
        div[u] = (2.0 / ((double)R * (double)(R - 1))) * s;
    }
}

// Shared host checks of a frames vector: returns sum(frames) or -1 (error set, `who` first).
long long check_frames(const char* who, const int32_t* frames, int U, int Tmax /*0: no upper bound*/) {
    if (!frames) { eg_set_error("%s: null frames", who); return -1; }
    if (U < 1 || U > MAX_U) { eg_set_error("%s: U=%d (1..%d)", who, U, MAX_U); return -1; }
    long long sum = 0;
    for (int u = 0; u < U; ++u) {
        if (frames[u] < 1 || (Tmax > 0 && frames[u] > Tmax)) {
            if (Tmax > 0) eg_set_error("%s: frames[%d]=%d (1..Tmax=%d)", who, u, frames[u], Tmax);
            else eg_set_error("%s: frames[%d]=%d (need >= 1)", who, u, frames[u]);
            return -1;
        }
        sum += frames[u];
    }
    if (sum >= (1ll << 31)) { eg_set_error("%s: sum(frames)=%lld: index range (< 2^31)", who, sum); return -1; }
    return sum;
}

long long distance_bytes(const char* who, const int32_t* frames, int U, int R) {
    const long long sum = check_frames(who, frames, U, 0);
    if (sum < 0) return 0;
    if (R < 2 || R > MAXR) { eg_set_error("%s: draws=%d (2..%d)", who, R, MAXR); return 0; }
    const long long slots = sum / CH + U;
    return slots * (R * (R - 1) / 2) * (long long)sizeof(double);
}

}  // namespace

extern "C" int64_t eg_take_meta_ints(int32_t recordings) { return recordings < 1 || recordings > MAX_U ? 0 : 2 * (int64_t)recordings; }

extern "C" int eg_take_meta(const int32_t* frames, int32_t recordings, int32_t* meta) {
    if (check_frames("eg_take_meta", frames, recordings, 0) < 0) return EG_ERR_BAD_ARG;
    EG_REQUIRE(meta, EG_ERR_BAD_ARG, "eg_take_meta: null meta");
    int32_t off = 0;
    for (int u = 0; u < recordings; ++u) {
        meta[u] = frames[u];
        meta[recordings + u] = off;
        off += frames[u];
    }
    return EG_OK;
}

extern "C" int eg_track_rows_pack(const float* track, int32_t U, int32_t R, int32_t Tmax, int32_t D, const int32_t* frames,
                                  const int32_t* d_meta, float* rows, void* stream) {
    const char* who = "eg_track_rows_pack";
    EG_REQUIRE(track, EG_ERR_BAD_ARG, "%s: null track", who);
    EG_REQUIRE(d_meta, EG_ERR_BAD_ARG, "%s: null d_meta", who);
    EG_REQUIRE(rows, EG_ERR_BAD_ARG, "%s: null rows", who);
    EG_REQUIRE(eg_aligned16(rows), EG_ERR_ALIGN, "%s: rows not 16-byte aligned", who);
    EG_REQUIRE(R >= 1 && R <= MAXR, EG_ERR_BAD_ARG, "%s: draws=%d (1..%d)", who, R, MAXR);
    EG_REQUIRE(Tmax >= 1, EG_ERR_BAD_ARG, "%s: Tmax=%d (need >= 1)", who, Tmax);
    EG_REQUIRE(D >= 1, EG_ERR_BAD_ARG, "%s: pose_dim=%d (need >= 1)", who, D);
    const long long sum = check_frames(who, frames, U, Tmax);
    if (sum < 0) return EG_ERR_BAD_ARG;
    const int Q = (D + 3) / 4;
    EG_REQUIRE((double)R * (double)sum * (4.0 * Q) < 1099511627776.0, EG_ERR_UNSUPPORTED, "%s: N*Dpad=%lld*%d: index range (< 2^40)", who,
               R * sum, 4 * Q);
    int maxf = 0;
    for (int u = 0; u < U; ++u) maxf = frames[u] > maxf ? frames[u] : maxf;
    const long long per = (long long)R * maxf * Q;              // quads of the longest recording
    long long gx = (per + 255) / 256;
    const long long cap = U >= 4096 ? 1 : 4096 / U;             // about 4096 workgroups in all, the rest by the grid stride
    gx = gx < 1 ? 1 : (gx > cap ? cap : gx);
    const bool vec = D % 4 == 0 && eg_aligned16(track);
    const bool small = per <= 0x7fffffffll - 4096ll * 256;      // i + gridDim.x*256 stays inside 32 bits
    const dim3 grid((unsigned)gx, (unsigned)U), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    f4* out = reinterpret_cast<f4*>(rows);
    if (vec && small) hipLaunchKernelGGL((track_rows_pack_kernel<true, unsigned>), grid, block, 0, st, track, d_meta, out, U, R, Tmax, D, Q);
    else if (vec) hipLaunchKernelGGL((track_rows_pack_kernel<true, size_t>), grid, block, 0, st, track, d_meta, out, U, R, Tmax, D, Q);
    else if (small) hipLaunchKernelGGL((track_rows_pack_kernel<false, unsigned>), grid, block, 0, st, track, d_meta, out, U, R, Tmax, D, Q);
    else hipLaunchKernelGGL((track_rows_pack_kernel<false, size_t>), grid, block, 0, st, track, d_meta, out, U, R, Tmax, D, Q);
    return eg_check_launch("track_rows_pack");
}

extern "C" int64_t eg_take_distance_workspace_bytes(const int32_t* frames, int32_t recordings, int32_t draws) {
    return distance_bytes("eg_take_distance_workspace_bytes", frames, recordings, draws);
}

extern "C" int eg_take_distance(const float* feat, int32_t U, int32_t R, int32_t K, const int32_t* frames, const int32_t* d_meta, int32_t span,
                                void* workspace, int64_t workspace_bytes, double* distance, double* diversity, void* stream) {
    const char* who = "eg_take_distance";
    const void* ptrs[5] = {feat, d_meta, workspace, distance, diversity};
    const char* names[5] = {"feat", "d_meta", "workspace", "distance", "diversity"};
    for (int i = 0; i < 5; ++i) EG_REQUIRE(ptrs[i], EG_ERR_BAD_ARG, "%s: null %s", who, names[i]);
    for (int i = 0; i < 5; ++i) EG_REQUIRE(i == 1 || eg_aligned16(ptrs[i]), EG_ERR_ALIGN, "%s: %s not 16-byte aligned", who, names[i]);
    const long long need = distance_bytes(who, frames, U, R);
    if (need <= 0) return EG_ERR_BAD_ARG;
    EG_REQUIRE(K >= 4 && K % 4 == 0, EG_ERR_BAD_ARG, "%s: feat_dim=%d (a multiple of 4, >= 4)", who, K);
    long long sum = 0;
    int maxf = 0;
    for (int u = 0; u < U; ++u) { sum += frames[u]; maxf = frames[u] > maxf ? frames[u] : maxf; }
    EG_REQUIRE((double)R * (double)sum * (double)K < 1099511627776.0, EG_ERR_UNSUPPORTED, "%s: N*K=%lld*%d: index range (< 2^40)", who, R * sum, K);
    EG_REQUIRE(workspace_bytes >= need, EG_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes, need);
    const long long gx = (long long)((maxf + CH - 1) / CH) * (R - 1);
    EG_REQUIRE(gx <= 0x7fffffffll, EG_ERR_UNSUPPORTED, "%s: %lld workgroups per recording: grid range", who, gx);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const f4* fq = reinterpret_cast<const f4*>(feat);
    double* ws = static_cast<double*>(workspace);
    const dim3 grid((unsigned)gx, (unsigned)U), block(256);
    if (K / 4 * CH <= REG_QUADS * 256) hipLaunchKernelGGL(take_distance_kernel<true>, grid, block, 0, st, fq, d_meta, ws, U, R, K / 4);
    else hipLaunchKernelGGL(take_distance_kernel<false>, grid, block, 0, st, fq, d_meta, ws, U, R, K / 4);
    int rc = eg_check_launch("take_distance");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(take_finish_kernel, dim3((unsigned)U), block, 0, st, ws, d_meta, distance, diversity, U, R, span);
    return eg_check_launch("take_finish");
}
